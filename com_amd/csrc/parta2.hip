// PartA2FCHead's RoI-aware pooling for the whole stacked batch, straight to sparse rows (gfx950).  C ABI: include/pcd_ops.h
// (f8).  Replaces roiaware_pool (pcdet/models/roi_heads/partA2_head.py:104-151: a host loop over frames with two
// RoIAwarePool3d calls each) and the nonzero() / gather of forward (:184-195).
//
// The contract is roiaware.hip's: a voxel's list is its frame's points in ascending index, cut after max_pts_each_voxel - 1
// entries; avg divides the sum in list order by the number listed, max takes the first strict maximum.  What is new is
// where the lists live.  One workgroup per RoI walks the points 1024 at a time, exactly as ra_collect_kernel does (all four
// waves test their points, wave 0 appends in point order with ballot ranks), twice:
//   plan   : voxel counters and the four avg sums of the part features in LDS; a voxel is a ROW when the fp32 sum of its
//            four pooled part features is non-zero.  Leaves count | row flag per voxel, and rows / listed points per RoI.
//   scan   : one workgroup: exclusive offsets of the RoIs' rows and list entries, the totals, the fake path (fewer than
//            three rows: one row per RoI at cell (0, 0, 0)) and the overflow flags.
//   write  : the same walk, now appending into ONE compact entry list for the whole batch (CSR: per row a start and a
//            count), then coords, part_rows and the row records.
//   rows   : one thread per (row, channel), channel fastest: max + argmax of the RPN features over the row's entries; rows
//            behind the device row count are cleared.
// No [RoIs][voxels][max_pts] list, no [RoIs][points] mask, no dense pooled tensor: the only per-voxel array is one int32.
#include "common.h"
#include "roiaware_geom.h"

#include "pcd_ops.h"

#include <limits.h>

#define PA_PTS 1024             // points per pass of the walk (4 per thread)
// (PCD_PARTA2_MAX_POOL = 14: a counter and four sums per voxel in LDS, 54 KiB for 14^3 voxels)
#define PA_ROW_FLAG (1 << 30)

namespace {

struct PaScene {
    const float *rois;          // [batch][num_rois][7]
    const float *pc;            // [P][4] (bs_idx, x, y, z)
    const float *part;          // rows of 3, part_stride apart
    const float *score;         // [P]
    long long part_stride;
    float thresh;
    int num_rois, P, pool, mpv;
};

// state words (device int32 [PCD_PARTA2_STATE_WORDS])
enum { PA_ROWS = 0, PA_ROWS_ALL = 1, PA_LISTED = 2, PA_FAKE = 3 };

__device__ __forceinline__ void pa_part_of(const PaScene &s, int idx, float f[4]) {
    // partA2_head.py:121-125: (part offset or xyz, score), the first three zeroed where score < thresh (strict)
    const float sc = s.score[idx];
    const float *p = s.part + (size_t)idx * s.part_stride;
    const bool masked = sc < s.thresh;
    f[0] = masked ? 0.f : p[0];
    f[1] = masked ? 0.f : p[1];
    f[2] = masked ? 0.f : p[2];
    f[3] = sc;
}

// WRITE == false (plan): vox[roi][v] = count | row flag, roi_cnt[0][roi] = rows, roi_cnt[1][roi] = listed points.
// WRITE == true: entries, coords, part_rows, row_ent for the RoI's rows.
template <bool WRITE>
__global__ __launch_bounds__(256) void pa_walk_kernel(PaScene s, int total_rois, int *__restrict__ vox, int *__restrict__ roi_cnt,
                                                      const int *__restrict__ offs, const int *__restrict__ state, int max_rows,
                                                      int max_listed, int *__restrict__ coords, float *__restrict__ part_rows,
                                                      int *__restrict__ row_ent, int *__restrict__ entries) {
    extern __shared__ int s_dyn[];                    // plan: cnt [V], sum [4 V];  write: cnt [V], base [V]
    __shared__ int s_vox[PA_PTS];
    __shared__ int s_scan[4];
    __shared__ int s_tot[2];
    const int roi = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nvox = s.pool * s.pool * s.pool;
    int *s_cnt = s_dyn;
    float *s_sum = (float *)(s_dyn + nvox);           // plan
    int *s_base = s_dyn + nvox;                       // write
    const float frame = (float)(roi / s.num_rois);
    const float *r = s.rois + (size_t)roi * 7;
    const RaBox box = ra_prepare(r, RA_MARGIN_DEVICE);
    const float dx = r[3], dy = r[4], dz = r[5];
    const float x_res = __fdiv_rn(dx, (float)s.pool), y_res = __fdiv_rn(dy, (float)s.pool), z_res = __fdiv_rn(dz, (float)s.pool);
    int *V = vox + (size_t)roi * nvox;
    int ent0 = 0;
    if (WRITE) {
        ent0 = offs[total_rois + 1 + roi];
        // exclusive offsets of the voxels' lists inside the RoI's piece of the entry list
        int carry = 0;
        for (int v0 = 0; v0 < nvox; v0 += 256) {
            const int v = v0 + tid;
            const int c = v < nvox ? (V[v] & (PA_ROW_FLAG - 1)) : 0;
            int tot;
            const int ex = block_exclusive_scan(c, s_scan, tot);
            if (v < nvox) s_base[v] = carry + ex;
            carry += tot;
        }
    }
    for (int v = tid; v < nvox; v += 256) {
        s_cnt[v] = 0;
        if (!WRITE) {
            s_sum[v * 4] = 0.f;
            s_sum[v * 4 + 1] = 0.f;
            s_sum[v * 4 + 2] = 0.f;
            s_sum[v * 4 + 3] = 0.f;
        }
    }
    if (tid < 2) s_tot[tid] = 0;
    __syncthreads();
    const u64 lower = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int base = 0; base < s.P; base += PA_PTS) {
#pragma unroll
        for (int j = 0; j < PA_PTS / 256; ++j) {
            const int k = base + j * 256 + tid;
            int v = -1;
            if (k < s.P) {
                const float *p = s.pc + (size_t)k * 4;
                if (p[0] == frame) {                                       // (batch_idx == bs_idx)
                    float lx, ly;
                    if (ra_point_in_box(box, p[1], p[2], p[3], lx, ly)) {
                        const float lz = p[3] - box.cz;
                        v = (ra_voxel_index(lx, dx, x_res, s.pool) * s.pool + ra_voxel_index(ly, dy, y_res, s.pool)) * s.pool +
                            ra_voxel_index(lz, dz, z_res, s.pool);
                    }
                }
            }
            s_vox[j * 256 + tid] = v;
        }
        __syncthreads();
        if (tid < 64) {
            // wave 0 appends in point order: within a 64-point piece the lanes of one voxel are ranked by ballots
            for (int k0 = 0; k0 < PA_PTS; k0 += 64) {
                const int v = s_vox[k0 + lane];
                u64 act = __ballot(v >= 0);
                if (!act) continue;
                const int idx = base + k0 + lane;
                float f[4] = {0.f, 0.f, 0.f, 0.f};
                if (!WRITE && v >= 0) pa_part_of(s, idx, f);
                while (act) {
                    const int leader = __ffsll((long long)act) - 1;
                    const int lv = __shfl(v, leader, 64);
                    const u64 same = __ballot(v == lv);
                    const int have = s_cnt[lv];
                    if (WRITE) {
                        if (v == lv) {
                            const int pos = have + __popcll(same & lower);
                            const long long e = (long long)ent0 + s_base[lv] + pos;
                            if (pos < s.mpv - 1 && e < (long long)max_listed) entries[e] = idx;
                        }
                    } else {
                        // the avg sums in list order (every lane runs the same loop: `same` is wave-uniform)
                        float a0 = s_sum[lv * 4], a1 = s_sum[lv * 4 + 1], a2 = s_sum[lv * 4 + 2], a3 = s_sum[lv * 4 + 3];
                        u64 m = same;
                        for (int taken = have; m && taken < s.mpv - 1; ++taken) {
                            const int j = __ffsll((long long)m) - 1;
                            a0 += __shfl(f[0], j, 64);
                            a1 += __shfl(f[1], j, 64);
                            a2 += __shfl(f[2], j, 64);
                            a3 += __shfl(f[3], j, 64);
                            m &= m - 1;
                        }
                        if (lane == leader) {
                            s_sum[lv * 4] = a0;
                            s_sum[lv * 4 + 1] = a1;
                            s_sum[lv * 4 + 2] = a2;
                            s_sum[lv * 4 + 3] = a3;
                        }
                    }
                    if (lane == leader) s_cnt[lv] = min(have + __popcll(same), s.mpv - 1);
                    act &= ~same;
                }
            }
        }
        __syncthreads();
    }
    if (!WRITE) {
        int rows = 0, listed = 0;
        for (int v = tid; v < nvox; v += 256) {
            const int c = s_cnt[v];
            int flag = 0;
            if (c > 0) {
                const float t = (float)c;
                const float p0 = __fdiv_rn(s_sum[v * 4], t), p1 = __fdiv_rn(s_sum[v * 4 + 1], t);
                const float p2 = __fdiv_rn(s_sum[v * 4 + 2], t), p3 = __fdiv_rn(s_sum[v * 4 + 3], t);
                if (((p0 + p1) + p2) + p3 != 0.f) flag = PA_ROW_FLAG;       // pooled_part_features.sum(dim=-1).nonzero()
            }
            V[v] = c | flag;
            rows += flag != 0;
            listed += c;
        }
        if (rows) atomicAdd(&s_tot[0], rows);                                // integers: order independent
        if (listed) atomicAdd(&s_tot[1], listed);
        __syncthreads();
        if (tid < 2) roi_cnt[tid * total_rois + roi] = s_tot[tid];
    } else {
        const bool fake = state[PA_FAKE] != 0;
        const int row0 = fake ? roi : offs[roi];
        int carry = 0;
        for (int v0 = 0; v0 < nvox; v0 += 256) {
            const int v = v0 + tid;
            const int word = v < nvox ? V[v] : 0;
            const bool emit = fake ? v == 0 : (word & PA_ROW_FLAG) != 0;
            int tot;
            const int rank = block_exclusive_scan(emit ? 1 : 0, s_scan, tot);
            const int row = row0 + (fake ? 0 : carry + rank);
            carry += tot;
            if (!emit || row >= max_rows) continue;
            const int c = word & (PA_ROW_FLAG - 1);
            const long long e0 = (long long)ent0 + s_base[v];
            const int have = (int)max(0ll, min((long long)c, (long long)max_listed - e0));   // (all of c unless the list overflowed)
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < have; ++k) {                                 // list order: the plan's sums, bit for bit
                float f[4];
                pa_part_of(s, entries[e0 + k], f);
                a[0] += f[0];
                a[1] += f[1];
                a[2] += f[2];
                a[3] += f[3];
            }
            const float t = (float)c;
            float4 pooled = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c > 0) pooled = make_float4(__fdiv_rn(a[0], t), __fdiv_rn(a[1], t), __fdiv_rn(a[2], t), __fdiv_rn(a[3], t));
            const int z = v % s.pool, y = (v / s.pool) % s.pool, x = v / (s.pool * s.pool);
            ((int4 *)coords)[row] = make_int4(roi, x, y, z);
            ((float4 *)part_rows)[row] = pooled;
            ((int2 *)row_ent)[row] = make_int2((int)e0, have);
        }
    }
}

// one workgroup: offs[0][.] = exclusive row offsets, offs[1][.] = exclusive entry offsets (each total_rois + 1 long)
__global__ __launch_bounds__(256) void pa_scan_kernel(const int *__restrict__ roi_cnt, int total_rois, int max_rows, int max_listed,
                                                      int *__restrict__ offs, int *__restrict__ state, int *__restrict__ status) {
    __shared__ int s_scan[4];
    int carry_r = 0, carry_e = 0;
    for (int r0 = 0; r0 < total_rois; r0 += 256) {
        const int r = r0 + (int)threadIdx.x;
        const int nr = r < total_rois ? roi_cnt[r] : 0, ne = r < total_rois ? roi_cnt[total_rois + r] : 0;
        int tr, te;
        const int er = block_exclusive_scan(nr, s_scan, tr);
        const int ee = block_exclusive_scan(ne, s_scan, te);
        if (r < total_rois) {
            offs[r] = carry_r + er;
            offs[total_rois + 1 + r] = carry_e + ee;
        }
        carry_r += tr;
        carry_e += te;
    }
    if (threadIdx.x == 0) {
        offs[total_rois] = carry_r;
        offs[2 * total_rois + 1] = carry_e;
        const bool fake = carry_r < 3;                                       // partA2_head.py:186-191
        const int rows = fake ? total_rois : carry_r;
        state[PA_ROWS] = min(rows, max_rows);
        state[PA_ROWS_ALL] = rows;
        state[PA_LISTED] = carry_e;
        state[PA_FAKE] = fake ? 1 : 0;
        if (status && (rows > max_rows || carry_e > max_listed)) status[0] |= (rows > max_rows ? 1 : 0) | (carry_e > max_listed ? 2 : 0);
    }
}

// one thread per (row, channel), channel fastest: max-pool the RPN features over the row's entries; rows behind the device
// row count are cleared (coords and part_rows too)
__global__ __launch_bounds__(256) void pa_rows_kernel(const float *__restrict__ feat, int C, int P, const int *__restrict__ state,
                                                      int max_rows, const int *__restrict__ row_ent, const int *__restrict__ entries,
                                                      int *__restrict__ coords, float *__restrict__ part_rows,
                                                      float *__restrict__ rpn_rows, int *__restrict__ argmax) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)max_rows * C) return;
    const int row = (int)(i / C), c = (int)(i - (size_t)row * C);
    if (row >= state[PA_ROWS]) {
        rpn_rows[i] = 0.f;
        argmax[i] = -1;
        if (c == 0) {
            ((int4 *)coords)[row] = make_int4(0, 0, 0, 0);
            ((float4 *)part_rows)[row] = make_float4(0.f, 0.f, 0.f, 0.f);
            ((int2 *)row_ent)[row] = make_int2(0, 0);
        }
        return;
    }
    const int2 e = ((const int2 *)row_ent)[row];
    int arg = -1;
    float mx = -INFINITY;
    for (int k = 0; k < e.y; ++k) {
        const int idx = entries[e.x + k];
        if ((unsigned)idx >= (unsigned)P) continue;
        const float f = feat[(size_t)idx * C + c];
        if (f > mx) {                                                        // the first strict maximum in list order
            mx = f;
            arg = idx;
        }
    }
    rpn_rows[i] = arg != -1 ? mx : 0.f;
    argmax[i] = arg;
}

// same thread layout: max through argmax; avg (the thread of channel 0) through the row's entries, the score column and the
// masked points receiving nothing
__global__ __launch_bounds__(256) void pa_grad_kernel(const float *__restrict__ g_part, const float *__restrict__ g_rpn, int C, int P,
                                                      const int *__restrict__ state, int max_rows, const int *__restrict__ row_ent,
                                                      const int *__restrict__ entries, const int *__restrict__ argmax,
                                                      const float *__restrict__ score, float thresh, float *__restrict__ d_part,
                                                      float *__restrict__ d_feat) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)max_rows * C) return;
    const int row = (int)(i / C), c = (int)(i - (size_t)row * C);
    if (row >= state[PA_ROWS]) return;
    const int a = argmax[i];
    if ((unsigned)a < (unsigned)P) atomicAdd(d_feat + (size_t)a * C + c, g_rpn[i]);
    if (c != 0 || !d_part) return;
    const int2 e = ((const int2 *)row_ent)[row];
    if (e.y <= 0) return;
    const float inv = __fdiv_rn(1.f, fmaxf((float)e.y, 1.f));
    const float g0 = g_part[(size_t)row * 4] * inv, g1 = g_part[(size_t)row * 4 + 1] * inv, g2 = g_part[(size_t)row * 4 + 2] * inv;
    for (int k = 0; k < e.y; ++k) {
        const int idx = entries[e.x + k];
        if ((unsigned)idx >= (unsigned)P || score[idx] < thresh) continue;
        atomicAdd(d_part + (size_t)idx * 3, g0);
        atomicAdd(d_part + (size_t)idx * 3 + 1, g1);
        atomicAdd(d_part + (size_t)idx * 3 + 2, g2);
    }
}

int scene_ok(int batch, int num_rois, int num_points, int pool, int mpv) {
    if (batch < 1 || num_rois < 1 || num_points < 0 || pool < 1 || mpv < 2) return PCD_ERR_INVALID_ARG;
    if ((long long)batch * num_rois > 65535 || pool > PCD_PARTA2_MAX_POOL || (long long)num_points * 4 >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    // the entry offsets are int32: a RoI lists a point at most once and a voxel at most mpv - 1 points
    const long long rois = (long long)batch * num_rois, nvox = (long long)pool * pool * pool;
    const long long listed = rois * (num_points < nvox * (mpv - 1) ? (long long)num_points : nvox * (mpv - 1));
    if (listed >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    return PCD_OK;
}

PaScene make_scene(const float *rois, int num_rois, const float *pc, int num_points, const float *part, long long part_stride,
                   const float *score, float thresh, int pool, int mpv) {
    PaScene s;
    s.rois = rois;
    s.pc = pc;
    s.part = part;
    s.score = score;
    s.part_stride = part_stride;
    s.thresh = thresh;
    s.num_rois = num_rois;
    s.P = num_points;
    s.pool = pool;
    s.mpv = mpv;
    return s;
}

}  // namespace

extern "C" int pcd_parta2_pool_plan(const float *rois, int batch, int num_rois, const float *point_coords, int num_points,
                                    const float *point_part, long long part_stride, const float *point_scores,
                                    float score_thresh, int pool_size, int max_pts_each_voxel, int max_rows, int max_listed,
                                    int *voxels, int *roi_counts, int *offsets, int *state, int *status, void *stream) {
    PCD_ENTER();
    const int rc = scene_ok(batch, num_rois, num_points, pool_size, max_pts_each_voxel);
    if (rc != PCD_OK) return rc;
    if (!rois || !voxels || !roi_counts || !offsets || !state || max_rows < 0 || max_listed < 0 || part_stride < 3)
        return PCD_ERR_INVALID_ARG;
    if (num_points > 0 && (!point_coords || !point_part || !point_scores)) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int R = batch * num_rois, nvox = pool_size * pool_size * pool_size;
    const PaScene s = make_scene(rois, num_rois, point_coords, num_points, point_part, part_stride, point_scores, score_thresh,
                                 pool_size, max_pts_each_voxel);
    pa_walk_kernel<false><<<R, 256, (size_t)nvox * 5 * sizeof(int), st>>>(s, R, voxels, roi_counts, nullptr, nullptr, 0, 0, nullptr,
                                                                          nullptr, nullptr, nullptr);
    pa_scan_kernel<<<1, 256, 0, st>>>(roi_counts, R, max_rows, max_listed, offsets, state, status);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_parta2_pool_forward(const float *rois, int batch, int num_rois, const float *point_coords, int num_points,
                                       const float *point_part, long long part_stride, const float *point_scores,
                                       float score_thresh, const float *point_features, int channels, int pool_size,
                                       int max_pts_each_voxel, int max_rows, int max_listed, const int *voxels,
                                       const int *offsets, const int *state, int *coords, float *part_rows, float *rpn_rows,
                                       int *row_entries, int *entries, int *argmax, void *stream) {
    PCD_ENTER();
    const int rc = scene_ok(batch, num_rois, num_points, pool_size, max_pts_each_voxel);
    if (rc != PCD_OK) return rc;
    if (channels < 1 || max_rows < 0 || max_listed < 0 || part_stride < 3 || !rois || !voxels || !offsets || !state)
        return PCD_ERR_INVALID_ARG;
    if ((long long)num_points * channels >= (1ll << 31) || (long long)max_rows * channels >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    if (max_rows == 0) return PCD_OK;
    if (!coords || !part_rows || !rpn_rows || !row_entries || !argmax || (max_listed > 0 && !entries)) return PCD_ERR_INVALID_ARG;
    if (num_points > 0 && (!point_coords || !point_part || !point_scores || !point_features)) return PCD_ERR_INVALID_ARG;
    if (((uintptr_t)coords & 15) || ((uintptr_t)part_rows & 15) || ((uintptr_t)row_entries & 7)) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int R = batch * num_rois, nvox = pool_size * pool_size * pool_size;
    const PaScene s = make_scene(rois, num_rois, point_coords, num_points, point_part, part_stride, point_scores, score_thresh,
                                 pool_size, max_pts_each_voxel);
    pa_walk_kernel<true><<<R, 256, (size_t)nvox * 2 * sizeof(int), st>>>(s, R, const_cast<int *>(voxels), nullptr, offsets, state,
                                                                         max_rows, max_listed, coords, part_rows, row_entries,
                                                                         entries);
    const unsigned grid = (unsigned)(((size_t)max_rows * channels + 255) / 256);
    pa_rows_kernel<<<grid, 256, 0, st>>>(point_features, channels, num_points, state, max_rows, row_entries, entries, coords, part_rows,
                                         rpn_rows, argmax);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_parta2_pool_backward(const float *grad_part_rows, const float *grad_rpn_rows, int channels, int num_points,
                                        int max_rows, const int *state, const int *row_entries, const int *entries,
                                        const int *argmax, const float *point_scores, float score_thresh, float *grad_part,
                                        float *grad_features, void *stream) {
    PCD_ENTER();
    if (channels < 1 || num_points < 0 || max_rows < 0) return PCD_ERR_INVALID_ARG;
    if ((long long)num_points * channels >= (1ll << 31) || (long long)max_rows * channels >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    if (num_points == 0) return PCD_OK;
    if (!grad_features) return PCD_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    pcd_fill(grad_features, 0, (size_t)num_points * channels * sizeof(float), st);
    if (grad_part) pcd_fill(grad_part, 0, (size_t)num_points * 3 * sizeof(float), st);
    if (max_rows > 0) {
        if (!grad_rpn_rows || !state || !row_entries || !argmax || (grad_part && (!grad_part_rows || !entries || !point_scores)))
            return PCD_ERR_INVALID_ARG;
        const unsigned grid = (unsigned)(((size_t)max_rows * channels + 255) / 256);
        pa_grad_kernel<<<grid, 256, 0, st>>>(grad_part_rows, grad_rpn_rows, channels, num_points, state, max_rows, row_entries, entries,
                                             argmax, point_scores, score_thresh, grad_part, grad_features);
    }
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
