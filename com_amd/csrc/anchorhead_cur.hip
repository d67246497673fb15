// The COM curriculum on the anchor head (gfx950): difficulty groups, anchor groups, and the curriculum form of the fused
// anchor loss.  C ABI: include/pcd_ops.h (f3b, pcd_anchor_cur_*).
//
//   pcd_anchor_cur_cluster        pcdet/models/dense_heads/curri_anchor_head_single.py:43-96 and head_zoo.py:12-140 (the
//                                 four `cluster` methods; the value a box holds after all overwriting assignments)
//   pcd_anchor_cur_groups         target_assigner/curri_axis_aligned_target_assigner.py:246-311 under POS_FRACTION < 0: the
//                                 `groups` output, as one gather over pcd_anchor_assign_targets' box index
//   pcd_anchor_cur_loss_forward / anchor_head_curriculum.py:103-256 with pcdet/utils/loss_utils.py:79-331
//   pcd_anchor_cur_loss_backward  (CurriculumSigmoidFocalClassificationLoss: update_score, groups_confidence, forward)
//
// The forward is four launches: a statistics pass over the anchor groups (only grouped positives load a prediction), a
// one-block state update, the loss pass (the anchor heads' core in anchorhead_common.h under its cell-major layout,
// curriculum variant) and the ordered finish.  This file holds what only the curriculum has: the cluster, groups,
// statistics and state kernels, and the entry points.  Statistics
// are accumulated as 64-bit fixed point (2^-40) with integer atomics (in LDS per block, then one flush per block that
// holds a grouped positive): exact, hence independent of the order of the adds, hence bit-identical between runs.  No [B, N, C, 97] tensor exists.  Compiled with -ffp-contract=off.
#include "anchorhead_common.h"

#define CUR_GROUPS PCD_ANCHOR_CUR_GROUPS
#define CUR_ACCUM (3 + 2 * CUR_GROUPS)      // sum, sum of squares, count; group sums; group counts

namespace {

typedef unsigned long long u64t;

// ---- cluster(): one block.  Scalars are compared in float32 (torch casts a Python number to the tensor's dtype).
__global__ __launch_bounds__(256) void anc_cur_cluster_kernel(const float *__restrict__ gt, int total, int code,
                                                              const float *__restrict__ true_object,
                                                              const float *__restrict__ occupancy,
                                                              const float *__restrict__ facade, int variant,
                                                              long long *__restrict__ group) {
    __shared__ float s_max[256];
    float mx = -INFINITY;                                               // class_id.max() over the whole batch, on the device
    for (int i = threadIdx.x; i < total; i += 256) mx = fmaxf(mx, gt[(size_t)i * code + code - 1]);
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + d]);
        __syncthreads();
    }
    const bool one = s_max[0] == 1.0f;
    const float ped = one ? 1.0f : 2.0f, cyc = one ? 1.0f : 3.0f;
    const bool x2 = variant == PCD_ANCHOR_CUR_CLUSTER_CAR_X2;
    const float t0 = x2 ? 0.21f : (float)(0.21 * 5 / 12), t1 = x2 ? 0.41f : (float)(0.41 * 5 / 12),
                t2 = x2 ? 0.61f : (float)(0.61 * 5 / 12), t3 = x2 ? 0.81f : (float)(0.81 * 5 / 12);
    for (int i = threadIdx.x; i < total; i += 256) {
        const float *q = gt + (size_t)i * code;
        const float x = q[0], y = q[1];
        const float dist = sqrtf(x * x + y * y);
        const float length = q[3], cls = q[code - 1];
        const float occ = occupancy[i], fac = facade[i];
        int dbin;
        if (variant == PCD_ANCHOR_CUR_CLUSTER_X1)
            dbin = dist <= 15.0f ? 0 : (dist <= 30.0f ? 1 : (dist <= 45.0f ? 2 : (dist <= 60.0f ? 3 : (dist > 60.0f ? 4 : -1))));
        else
            dbin = dist <= 30.0f ? 0 : (dist <= 50.0f ? 1 : (dist > 50.0f ? 2 : -1));
        const int lbin = length <= 6.0f ? 0 : (length > 6.0f ? 1 : -1);
        const int fbin = fac == 3.0f ? 0 : (fac == 2.0f ? 1 : (fac == 1.0f ? 2 : (fac == 0.0f ? 3 : -1)));
        const int ocar = occ > 0.7f ? 0 : (occ > 0.5f ? 1 : (occ > 0.25f ? 2 : (occ <= 0.25f ? 3 : -1)));
        const int o5 = occ > t3 ? 0 : (occ > t2 ? 1 : (occ > t1 ? 2 : (occ > t0 ? 3 : (occ <= t0 ? 4 : -1))));
        const int nd5 = 5;
        const long long car = (dbin >= 0 && lbin >= 0 && fbin >= 0 && ocar >= 0) ? 1 + ((dbin * 2 + lbin) * 4 + fbin) * 4 + ocar : 0;
        const long long five = (dbin >= 0 && o5 >= 0) ? 1 + dbin * nd5 + o5 : 0;
        long long g = 0;
        if (true_object[i] == 1.0f) {
            if (variant == PCD_ANCHOR_CUR_CLUSTER_BASE) {                 // only the pedestrian loop is live (:78-85)
                if (cls == ped) g = five;
            } else if (variant == PCD_ANCHOR_CUR_CLUSTER_X1) {            // car, then pedestrian, then cyclist loop: the last writer
                if (cls == 1.0f) g = car;
                if ((cls == ped || cls == cyc) && five) g = five;
            } else if (variant == PCD_ANCHOR_CUR_CLUSTER_CAR) {
                if (cls == 1.0f) g = car;
            } else {
                if (cls == 1.0f) g = five;
            }
        }
        group[i] = g;
    }
}

// ---- groups of the anchors: positive -> its box's group, label 0 -> 0, ignored -> -1
__global__ __launch_bounds__(256) void anc_cur_groups_kernel(const int *__restrict__ labels, const int *__restrict__ gt_index,
                                                             const long long *__restrict__ group, int N, int M,
                                                             int *__restrict__ groups) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const size_t o = (size_t)b * N + n;
    const int label = labels[o];
    int g = label == 0 ? 0 : -1;
    if (label > 0) {
        const int j = gt_index[o];
        g = (j >= 0 && j < M) ? (int)group[(size_t)b * M + j] : 0;
    }
    groups[o] = g;
}

// ---- statistics pass (update_score :150-198 sums; groups_confidence :200-214)
__device__ __forceinline__ u64t fixed40(double v) { return (u64t)__double2ll_rn(v * 1099511627776.0); }

__global__ __launch_bounds__(256) void anc_cur_stats_kernel(CellMajor lay, int dtype, int H, int W, int A,
                                                            const int *__restrict__ groups, u64t *__restrict__ accum) {
    __shared__ u64t s_acc[CUR_ACCUM];
    const int N = H * W * A;
    const int b = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int g = n < N ? groups[(size_t)b * N + n] : 0;
    if (threadIdx.x < CUR_ACCUM) s_acc[threadIdx.x] = 0;
    if (!__syncthreads_or(g > 0)) return;                                // (block-uniform: most blocks hold no grouped positive)
    if (g > 0) {
        const AncGeom q = CellMajor::geom(n, H, W, A);
        const AncHead &m = lay.h;
        const long long off = (long long)b * m.strides[0][0] + (long long)q.y * m.strides[0][2] +
                              (long long)q.x * m.strides[0][3] + (long long)(q.g * m.num_class) * m.strides[0][1];
        const float p = 1.f / (1.f + expf(-load_el(m.map[0], dtype, off)));
        const u64t fp = fixed40((double)p);
        atomicAdd(s_acc + 0, fp);                                        // integer sums: exact in any order
        atomicAdd(s_acc + 1, fixed40((double)p * (double)p));
        atomicAdd(s_acc + 2, (u64t)1);
        if (g <= CUR_GROUPS) {
            atomicAdd(s_acc + 3 + (g - 1), fp);
            atomicAdd(s_acc + 3 + CUR_GROUPS + (g - 1), (u64t)1);
        }
    }
    __syncthreads();
    if (threadIdx.x < CUR_ACCUM && s_acc[threadIdx.x] != 0) atomicAdd(accum + threadIdx.x, s_acc[threadIdx.x]);
}

struct AncCurState {
    int ucl, norm;
    double offset, ema;
};

// ---- state update (:183-197), thresholds of this step (:240-247), confidence tensors; clears the accumulators
__global__ __launch_bounds__(256) void anc_cur_state_kernel(u64t *accum, AncCurState q, const float *__restrict__ epoch_table,
                                                            double *state, float *conf_sum, float *conf_num,
                                                            float *epoch_conf, float *epoch_num, float *saved) {
    const int t = threadIdx.x;
    const double unit = 1.0 / 1099511627776.0;
    if (t < CUR_GROUPS) {
        const float s = (float)((double)accum[3 + t] * unit), c = (float)accum[3 + CUR_GROUPS + t];
        conf_sum[t] = s;
        conf_num[t] = c;
        epoch_conf[t] += s;
        epoch_num[t] += c;
    }
    if (t == 0) {
        const double sum = (double)accum[0] * unit, sq = (double)accum[1] * unit, n = (double)accum[2];
        if (q.ucl && n > 0.0) {
            const double mean = sum / n;
            const double v = sq + n * mean * mean - 2.0 * mean * sum;
            const double sd = v <= 0.0 ? 0.0 : sqrt(v / n);
            if (state[2] == 0.0) {
                state[0] = mean;
                state[1] = sd;
                state[2] = 1.0;
            } else {
                state[0] = (1.0 - q.ema) * state[0] + q.ema * mean;
                state[1] = (1.0 - q.ema) * state[1] + q.ema * sd;
            }
        }
        double thr = 0.5, var = 0.2;                                     // no statistics yet (:243-246)
        if (state[2] != 0.0) {
            thr = state[0] + q.offset * state[1];
            var = state[1];
        }
        if (!q.norm) var = 1.0;
        saved[SV_THR] = (float)thr;
        saved[SV_VAR] = (float)var;
        saved[SV_HEIGHT] = epoch_table[0];
        saved[SV_ELONG] = epoch_table[1];
        saved[SV_GATE] = epoch_table[2];
        saved[5] = saved[6] = saved[7] = 0.f;
    }
    __syncthreads();
    if (t < CUR_ACCUM) accum[t] = 0;
}

bool cur_args(AncCurArgs &a, AncCurState *s, const PcdAnchorCurriculum *cur, const int *groups, const float *saved) {
    if (!cur || !groups || !saved) return false;
    a.q.mode = !cur->ucl ? ANC_CUR_OFF : (cur->sm ? ANC_CUR_SM : (cur->sma ? ANC_CUR_SMA : ANC_CUR_SIGMOID));
    a.q.oto = cur->oto;
    a.q.smt = cur->smt;
    a.q.pos_norm = cur->pos_norm;
    a.q.neg_norm = cur->neg_norm;
    a.groups = groups;
    a.saved = saved;
    if (s) {
        s->ucl = cur->ucl;
        s->norm = cur->norm;
        s->offset = cur->offset;
        s->ema = cur->ema;
    }
    return true;
}

}  // namespace

extern "C" int pcd_anchor_cur_cluster(const float *gt_boxes, int batch, int n_boxes, int code_size, const float *true_object,
                                      const float *occupancy_ratio, const float *facade_type, int variant, long long *group,
                                      void *stream) {
    PCD_ENTER();
    if (batch < 0 || n_boxes < 0 || code_size < 8) return PCD_ERR_INVALID_ARG;
    if (variant < PCD_ANCHOR_CUR_CLUSTER_BASE || variant > PCD_ANCHOR_CUR_CLUSTER_CAR_X2) return PCD_ERR_UNSUPPORTED;
    const long long total = (long long)batch * n_boxes;
    if (total == 0) return PCD_OK;
    if (!gt_boxes || !true_object || !occupancy_ratio || !facade_type || !group) return PCD_ERR_INVALID_ARG;
    if (total >= (1ll << 27)) return PCD_ERR_UNSUPPORTED;
    anc_cur_cluster_kernel<<<1, 256, 0, (hipStream_t)stream>>>(gt_boxes, (int)total, code_size, true_object, occupancy_ratio,
                                                               facade_type, variant, group);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_cur_groups(const int *box_cls_labels, const int *gt_index, const long long *group, int batch,
                                     int n_anchors, int n_boxes, int *groups, void *stream) {
    PCD_ENTER();
    if (!box_cls_labels || !gt_index || !groups || batch < 1 || n_anchors < 1 || n_boxes < 0 || (n_boxes > 0 && !group))
        return PCD_ERR_INVALID_ARG;
    if (batch > 65535 || (long long)batch * n_anchors >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    dim3 grid(pcd_div_up(n_anchors, 256), batch);
    anc_cur_groups_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(box_cls_labels, gt_index, group, n_anchors, n_boxes, groups);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_anchor_cur_loss_workspace_bytes(int batch, int height, int width, int n_kinds) {
    return loss_workspace_bytes(batch, height, width, n_kinds);
}

extern "C" int pcd_anchor_cur_loss_forward(const void *cls_preds, const void *box_preds, const void *dir_preds, int dtype,
                                           const long long *strides_host, const int *box_cls_labels,
                                           const float *box_reg_targets, const int *num_pos, const int *groups, int batch,
                                           int height, int width, int n_kinds, int num_class, int num_dir_bins,
                                           const float *kinds, const float *code_weights, float cls_weight, float loc_weight,
                                           float dir_weight, float dir_offset, const PcdAnchorCurriculum *cur,
                                           const float *epoch_table, double *state, unsigned long long *accum, float *conf_sum,
                                           float *conf_num, float *epoch_conf, float *epoch_num, float *saved, float *out,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    CellMajor m;
    AncLossCfg c;
    AncCurArgs a;
    AncCurState s;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, nullptr, nullptr, nullptr, dtype, strides_host, n_kinds, num_class) ||
        !box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights || !out ||
        !cur_args(a, &s, cur, groups, saved) || !epoch_table || !state || !accum || !conf_sum || !conf_num || !epoch_conf ||
        !epoch_num)
        return PCD_ERR_INVALID_ARG;
    if (num_class != 1) return PCD_ERR_UNSUPPORTED;          // the reference's get_loss cannot run with more (pcd_ops.h)
    if (!loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, 7, 0, num_dir_bins, dir_preds != nullptr, true, 1.f, 1.f,
                  cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    WsCarver ws(workspace, workspace_bytes);
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    float *partials = ws.take<float>((size_t)grid.x * grid.y * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    anc_cur_stats_kernel<<<grid, 256, 0, st>>>(m, dtype, height, width, n_kinds, groups, accum);
    anc_cur_state_kernel<<<1, 256, 0, st>>>(accum, s, epoch_table, state, conf_sum, conf_num, epoch_conf, epoch_num, saved);
    launch_loss_forward(m, c, grid, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, partials, out, a, st);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_anchor_cur_loss_backward(const void *cls_preds, const void *box_preds, const void *dir_preds, void *d_cls,
                                            void *d_box, void *d_dir, int dtype, const long long *strides_host,
                                            const int *box_cls_labels, const float *box_reg_targets, const int *num_pos,
                                            const int *groups, int batch, int height, int width, int n_kinds, int num_class,
                                            int num_dir_bins, const float *kinds, const float *code_weights, float cls_weight,
                                            float loc_weight, float dir_weight, float dir_offset,
                                            const PcdAnchorCurriculum *cur, const float *saved, const float *grad_out,
                                            void *stream) {
    PCD_ENTER();
    CellMajor m;
    AncLossCfg c;
    AncCurArgs a;
    if (!fill_maps(m, cls_preds, box_preds, dir_preds, d_cls, d_box, d_dir, dtype, strides_host, n_kinds, num_class) || !d_cls ||
        !d_box || (dir_preds && !d_dir) || !box_cls_labels || !box_reg_targets || !num_pos || !kinds || !code_weights ||
        !grad_out || !cur_args(a, nullptr, cur, groups, saved))
        return PCD_ERR_INVALID_ARG;
    if (num_class != 1) return PCD_ERR_UNSUPPORTED;
    if (!loss_cfg(c, dtype, batch, height, width, n_kinds, num_class, 7, 0, num_dir_bins, dir_preds != nullptr, true, 1.f, 1.f,
                  cls_weight, loc_weight, dir_weight, dir_offset))
        return PCD_ERR_UNSUPPORTED;
    dim3 grid(pcd_div_up(height * width * n_kinds, 256), batch);
    anc_loss_kernel<true, CellMajor, AncCurArgs><<<grid, 256, 0, (hipStream_t)stream>>>(
        m, c, box_cls_labels, box_reg_targets, num_pos, kinds, code_weights, grad_out, nullptr, a);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
