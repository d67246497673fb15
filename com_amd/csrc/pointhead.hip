// The point heads (PointHeadSimple, PointHeadBox, PointIntraPartOffsetHead) on the device (gfx950): targets, losses, box
// decoding.  C ABI: include/pcd_ops.h (f5); Python: com_amd/hotpath/point_head.py.
//
//   pcd_point_head_assign_targets_full   point_head_simple.py:21-48, point_head_box.py:32-59, point_intra_part_head.py:39-66
//                                = point_head_template.py:49-129 (assign_stack_targets with set_ignore_flag) + box_utils.py:
//                                187-200 (enlarge_box3d) for the whole stacked batch, with ret_box_labels
//                                (box_coder_utils.py:153-187) and / or ret_part_labels (:114-122) where their pointers are
//                                given: the one targets entry of all three heads
//   pcd_point_head_loss_forward / _backward   point_head_template.py:131-155 (get_cls_layer_loss) with loss_utils.py:10-74:
//                                PointHeadSimple's (one upstream gradient, see DESIGN.md 4.8 for why it stays)
//   pcd_point_head_full_loss_forward / _backward   point_head_template.py:131-191 with loss_utils.py:338-399: the cls, box and
//                                part losses in one pass; a head without a branch passes NULL for it
//   pcd_point_head_decode        point_head_template.py:193-207 + box_coder_utils.py:189-222
//
// Targets: one thread per point, the point-in-box test of roiaware.hip (roiaware_geom.h).  A GT row's plain and enlarged
// box are staged together in LDS (one sincos for both), and a workgroup walks the frames its points belong to (one, when the
// stacked points are sorted by frame).  The loss pieces (focal element, ordered block sums and finish) are the anchor heads'
// (anchorhead_common.h).
#include "anchorhead_common.h"
#include "roiaware_geom.h"

#include <limits.h>

namespace {

struct PhBox {
    RaBox in;                   // the GT box
    double tx_e, ty_e;          // the enlarged box: same centre and heading
    float hz_e;
    int cls;
};

// What the box / part heads add to the targets (PointHeadBox, PointIntraPartOffsetHead): the row of the winning box is
// remembered through the chunk loop, and the foreground points encode it.  PhNoRows compiles to the PointHeadSimple kernel.
#define PH_MAX_MEAN 16          // rows of the PointResidualCoder mean-size table

struct PhNoRows {
    static constexpr bool on = false;
};
struct PhRows {
    static constexpr bool on = true;
    float *box_labels;          // [N][8] or NULL
    float *part_labels;         // [N][3] or NULL
    const float *mean_size;     // [num_mean][3] (device) or NULL: use_mean_size == False
    int num_mean;
};

template <class Rows>
__global__ __launch_bounds__(256) void ph_assign_kernel(const float *__restrict__ pc, int N, const float *__restrict__ gt, int B, int M,
                                                        float ex, float ey, float ez, int num_class,
                                                        long long *__restrict__ labels, int *__restrict__ num_pos, Rows rows) {
    __shared__ PhBox s_box[RA_CHUNK];
    __shared__ int s_lo, s_hi;
    __shared__ int s_cnt[4];
    int win = 0;                                                          // row of the first containing box in its frame
    float win_lx = 0.f, win_ly = 0.f;                                     // the point in that box's frame (ra_local)
    const int n = blockIdx.x * 256 + threadIdx.x;
    const bool valid = n < N;
    if (threadIdx.x == 0) {
        s_lo = INT_MAX;
        s_hi = -1;
    }
    __syncthreads();
    int bs = -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (valid) {
        const float *p = pc + (size_t)n * 4;
        const float fb = p[0];
        if (fb >= 0.f && fb < (float)B && fb == (float)(int)fb) bs = (int)fb;   // (bs_idx == k): other rows match no frame
        x = p[1];
        y = p[2];
        z = p[3];
        if (bs >= 0) {
            atomicMin(&s_lo, bs);
            atomicMax(&s_hi, bs);
        }
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;
    bool fg = false, ext = false;
    int cls = 0;
    for (int f = lo; f <= hi; ++f) {
        for (int m0 = 0; m0 < M; m0 += RA_CHUNK) {
            const int cnt = min(RA_CHUNK, M - m0);
            __syncthreads();
            if ((int)threadIdx.x < cnt) {
                const float *g = gt + ((size_t)f * M + m0 + threadIdx.x) * 8;
                PhBox q;
                q.in = ra_prepare(g, RA_MARGIN_DEVICE);
                RaBox e = q.in;                                          // enlarge_box3d: widths added to every row,
                ra_extents(e, g[3] + ex, g[4] + ey, g[5] + ez, RA_MARGIN_DEVICE);   // zero padding rows included
                q.tx_e = e.tx;
                q.ty_e = e.ty;
                q.hz_e = e.hz;
                q.cls = (int)g[7];
                s_box[threadIdx.x] = q;
            }
            __syncthreads();
            if (bs != f || (fg && ext)) continue;
            for (int j = 0; j < cnt; ++j) {
                const PhBox &q = s_box[j];
                const bool zi = !fg && ra_z_inside(z, q.in.cz, q.in.hz);
                const bool ze = !ext && ra_z_inside(z, q.in.cz, q.hz_e);
                if (!zi && !ze) continue;
                float lx, ly;
                ra_local(q.in, x, y, lx, ly);
                if (zi && ra_xy_inside(lx, ly, q.in.tx, q.in.ty)) {        // the FIRST containing box gives the class
                    fg = true;
                    cls = q.cls;
                    if constexpr (Rows::on) {
                        win = m0 + j;
                        win_lx = lx;
                        win_ly = ly;
                    }
                }
                if (ze && ra_xy_inside(lx, ly, q.tx_e, q.ty_e)) ext = true;
                if (fg && ext) break;
            }
        }
    }
    // point_head_template.py:91-92, :101-102: ignored where fg XOR inside an enlarged box, then the foreground's class
    int label = 0;
    if (fg != ext) label = -1;
    if (fg) label = num_class == 1 ? 1 : cls;
    if (valid) labels[n] = (long long)label;
    if constexpr (Rows::on) {
        __shared__ float s_mean[PH_MAX_MEAN * 3];
        if (rows.mean_size && (int)threadIdx.x < rows.num_mean * 3) s_mean[threadIdx.x] = rows.mean_size[threadIdx.x];
        __syncthreads();
        if (valid) {
            float bl[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float pl[3] = {0.f, 0.f, 0.f};
            if (fg) {                                                    // every fg_flag point, whatever its class (:105-122)
                const float *g = gt + ((size_t)bs * M + win) * 8;
                float dxg = g[3], dyg = g[4], dzg = g[5];
                if (rows.box_labels) {
                    // PointResidualCoder.encode_torch (box_coder_utils.py:153-187); its clamp is in place, so the part
                    // labels below divide by the clamped sizes too when both are asked for
                    dxg = fmaxf(dxg, 1e-5f);
                    dyg = fmaxf(dyg, 1e-5f);
                    dzg = fmaxf(dzg, 1e-5f);
                    if (rows.mean_size) {
                        int k = (int)g[7] - 1;                           // column 7 even when num_class == 1
                        k = k < 0 ? 0 : (k > rows.num_mean - 1 ? rows.num_mean - 1 : k);   // clamped (the reference asserts)
                        const float dxa = s_mean[k * 3], dya = s_mean[k * 3 + 1], dza = s_mean[k * 3 + 2];
                        const float diagonal = sqrtf(dxa * dxa + dya * dya);
                        bl[0] = (g[0] - x) / diagonal;
                        bl[1] = (g[1] - y) / diagonal;
                        bl[2] = (g[2] - z) / dza;
                        bl[3] = logf(dxg / dxa);
                        bl[4] = logf(dyg / dya);
                        bl[5] = logf(dzg / dza);
                    } else {
                        bl[0] = g[0] - x;
                        bl[1] = g[1] - y;
                        bl[2] = g[2] - z;
                        bl[3] = logf(dxg);
                        bl[4] = logf(dyg);
                        bl[5] = logf(dzg);
                    }
                    bl[6] = cosf(g[6]);
                    bl[7] = sinf(g[6]);
                }
                // :114-122: the point in the box's frame (rotate_points_along_z by -heading = ra_local) over the sizes + 0.5
                pl[0] = win_lx / dxg + 0.5f;
                pl[1] = win_ly / dyg + 0.5f;
                pl[2] = (z - g[2]) / dzg + 0.5f;
            }
            if (rows.box_labels) {
                float4 *o = (float4 *)(rows.box_labels + (size_t)n * 8);
                o[0] = make_float4(bl[0], bl[1], bl[2], bl[3]);
                o[1] = make_float4(bl[4], bl[5], bl[6], bl[7]);
            }
            if (rows.part_labels) {
                float *o = rows.part_labels + (size_t)n * 3;
                o[0] = pl[0];
                o[1] = pl[1];
                o[2] = pl[2];
            }
        }
    }
    const int wave_cnt = __popcll(__ballot(valid && label > 0));
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (c) atomicAdd(num_pos, c);                                    // integer: order independent
    }
}

__global__ void ph_clear_kernel(int *num_pos) { num_pos[0] = 0; }

// get_cls_layer_loss for ONE point over its num_class logits at logits[base ...]; the focal element is the anchor heads'
// (focal_el).  GRAD == false: returns the point's weighted loss.  GRAD == true: writes d loss / d logits of the point's row
// (every element) scaled by `upstream` and cls_w.
template <bool GRAD>
__device__ __forceinline__ float ph_cls_point(const void *__restrict__ logits, void *__restrict__ d_logits, int dtype,
                                              long long base, long long label, int num_class,
                                              const int *__restrict__ num_pos, float upstream, float cls_w) {
    // cls_weights = ((label == 0) + (label > 0)) / clamp(pos, 1)          (:135-139)
    const float w = label >= 0 ? 1.f / fmaxf((float)num_pos[0], 1.f) : 0.f;
    const long long tcls = label > 0 ? label - 1 : -1;                     // the one-hot without its column 0 (:141-143)
    float l = 0.f, up = 0.f;
    if (GRAD) up = upstream * w;
    for (int j = 0; j < num_class; ++j) {
        const long long off = base + j;
        if (label < 0) {
            if (GRAD) store_el(d_logits, dtype, off, 0.f);
            continue;
        }
        const float xv = load_el(logits, dtype, off);
        const float t = ((long long)j == tcls) ? 1.f : 0.f;
        if (!GRAD) l += focal_el<false>(xv, t) * w;
        else store_el(d_logits, dtype, off, focal_el<true>(xv, t) * up * cls_w);
    }
    return l;
}

// PointHeadSimple's loss: one thread per point.  GRAD == false: per-block partial sums (slot 0 of the three block_sum3
// carries).  GRAD == true: d loss / d logits, every element written.
template <bool GRAD>
__global__ __launch_bounds__(256) void ph_loss_kernel(const void *__restrict__ logits, void *__restrict__ d_logits, int dtype,
                                                      long long row_stride, const long long *__restrict__ labels,
                                                      const int *__restrict__ num_pos, int N, int num_class, float cls_w,
                                                      const float *__restrict__ grad_out, float *__restrict__ partials) {
    __shared__ float s_red[12];
    const int n = blockIdx.x * 256 + threadIdx.x;
    float l = 0.f;
    if (n < N) l = ph_cls_point<GRAD>(logits, d_logits, dtype, (long long)n * row_stride, labels[n], num_class, num_pos,
                                      GRAD ? grad_out[0] : 0.f, cls_w);
    if (!GRAD) block_sum3(l, 0.f, 0.f, s_red, partials + (size_t)blockIdx.x * 3);
}

// The three losses of PointHeadBox / PointIntraPartOffsetHead in one pass, one thread per point: the classification term
// is ph_cls_point, the box term the anchor heads' smooth-L1 element (beta 1/9, nan targets ignored, code weights), the
// part term binary cross entropy from the LOGIT.  A NULL box / part prediction skips its term.  GRAD == false: per-block
// partial sums in the three block_sum3 slots.  GRAD == true: the three gradients, every element written; grad_out holds the
// upstream gradients of out[0..4) (total, cls, box, part), so a term receives grad_out[0] + grad_out[1 + term].
struct PhPreds {
    const void *cls, *box, *part;
    void *d_cls, *d_box, *d_part;
    long long cls_stride, box_stride, part_stride;
    int dtype;
};

template <bool GRAD>
__global__ __launch_bounds__(256) void ph_full_loss_kernel(PhPreds q, const long long *__restrict__ labels,
                                                           const float *__restrict__ box_labels,
                                                           const float *__restrict__ part_labels,
                                                           const int *__restrict__ num_pos, const float *__restrict__ code_weights,
                                                           int N, int num_class, float cls_w, float box_w, float part_w,
                                                           const float *__restrict__ grad_out, float *__restrict__ partials) {
    __shared__ float s_red[12];
    const int n = blockIdx.x * 256 + threadIdx.x;
    float l_cls = 0.f, l_box = 0.f, l_part = 0.f;
    if (n < N) {
        const long long label = labels[n];
        const bool pos = label > 0;
        const float inv = 1.f / fmaxf((float)num_pos[0], 1.f);
        // ---- classification (point_head_template.py:131-155): PointHeadSimple's
        l_cls = ph_cls_point<GRAD>(q.cls, q.d_cls, q.dtype, (long long)n * q.cls_stride, label, num_class, num_pos,
                                   GRAD ? grad_out[0] + grad_out[1] : 0.f, cls_w);
        // ---- box (:172-191 with WeightedSmoothL1Loss, loss_utils.py:372-399): weights (label > 0) / max(num_pos, 1)
        if (q.box) {
            const float beta = 1.0f / 9.0f;
            float up = 0.f;
            if (GRAD) up = (grad_out[0] + grad_out[2]) * inv;
            for (int j = 0; j < 8; ++j) {
                const long long off = (long long)n * q.box_stride + j;
                if (!pos) {
                    if (GRAD) store_el(q.d_box, q.dtype, off, 0.f);
                    continue;
                }
                const float pv = load_el(q.box, q.dtype, off), tv = box_labels[(size_t)n * 8 + j], cw = code_weights[j];
                const bool nan_t = tv != tv;                             // :385: nan targets are ignored
                const float diff = nan_t ? 0.f : (pv - tv) * cw;
                const float ad = fabsf(diff);
                if (!GRAD) {
                    l_box += (ad < beta ? 0.5f * (ad * ad) / beta : ad - 0.5f * beta) * inv;
                } else {
                    const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                    const float dl = ad < beta ? diff / beta : sgn;
                    store_el(q.d_box, q.dtype, off, nan_t ? 0.f : dl * cw * up * box_w);
                }
            }
        }
        // ---- part (:157-170): F.binary_cross_entropy(sigmoid(p), t) = t softplus(-p) + (1 - t) softplus(p), each log term
        //      capped at 100 as binary_cross_entropy caps it; over the 3 columns of the positives / (3 max(num_pos, 1))
        if (q.part) {
            const float w3 = inv / 3.f;
            float up = 0.f;
            if (GRAD) up = (grad_out[0] + grad_out[3]) * w3;
            for (int j = 0; j < 3; ++j) {
                const long long off = (long long)n * q.part_stride + j;
                if (!pos) {
                    if (GRAD) store_el(q.d_part, q.dtype, off, 0.f);
                    continue;
                }
                const float pv = load_el(q.part, q.dtype, off), t = part_labels[(size_t)n * 3 + j];
                const float tail = log1pf(expf(-fabsf(pv)));
                const float sp_pos = fmaxf(pv, 0.f) + tail, sp_neg = fmaxf(-pv, 0.f) + tail;   // -log(1 - s), -log(s)
                if (!GRAD) {
                    l_part += (t * fminf(sp_neg, 100.f) + (1.f - t) * fminf(sp_pos, 100.f)) * w3;
                } else {
                    const float s = 1.f / (1.f + expf(-pv));
                    const float d = t * (sp_neg < 100.f ? s - 1.f : 0.f) + (1.f - t) * (sp_pos < 100.f ? s : 0.f);
                    store_el(q.d_part, q.dtype, off, d * up * part_w);
                }
            }
        }
    }
    if (!GRAD) block_sum3(l_cls, l_box, l_part, s_red, partials + (size_t)blockIdx.x * 3);
}

// generate_predicted_boxes (point_head_template.py:193-207) + PointResidualCoder.decode_torch (box_coder_utils.py:189-222):
// one thread per point.  The class is the FIRST maximum of the point's logits + 1 (torch.max), or classes[n] when given.
__global__ __launch_bounds__(256) void ph_decode_kernel(const void *__restrict__ cls, long long cls_stride, int num_class,
                                                        const long long *__restrict__ classes, const void *__restrict__ enc,
                                                        long long enc_stride, int dtype, const float *__restrict__ points,
                                                        long long point_stride, const float *__restrict__ mean_size, int num_mean,
                                                        int N, float *__restrict__ boxes) {
    __shared__ float s_mean[PH_MAX_MEAN * 3];
    if (mean_size && (int)threadIdx.x < num_mean * 3) s_mean[threadIdx.x] = mean_size[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = load_el(enc, dtype, (long long)n * enc_stride + j);
    const float *p = points + (long long)n * point_stride;
    const float xa = p[0], ya = p[1], za = p[2];
    float *o = boxes + (size_t)n * 7;
    if (mean_size) {
        long long c;
        if (classes) {
            c = classes[n] - 1;
        } else {
            c = 0;
            float mx = load_el(cls, dtype, (long long)n * cls_stride);
            for (int j = 1; j < num_class; ++j) {
                const float v = load_el(cls, dtype, (long long)n * cls_stride + j);
                if (v > mx) {
                    mx = v;
                    c = j;
                }
            }
        }
        const int k = c < 0 ? 0 : (c > num_mean - 1 ? num_mean - 1 : (int)c);   // clamped (the reference asserts)
        const float dxa = s_mean[k * 3], dya = s_mean[k * 3 + 1], dza = s_mean[k * 3 + 2];
        const float diagonal = sqrtf(dxa * dxa + dya * dya);
        o[0] = t[0] * diagonal + xa;
        o[1] = t[1] * diagonal + ya;
        o[2] = t[2] * dza + za;
        o[3] = expf(t[3]) * dxa;
        o[4] = expf(t[4]) * dya;
        o[5] = expf(t[5]) * dza;
    } else {
        o[0] = t[0] + xa;
        o[1] = t[1] + ya;
        o[2] = t[2] + za;
        o[3] = expf(t[3]);
        o[4] = expf(t[4]);
        o[5] = expf(t[5]);
    }
    o[6] = atan2f(t[7], t[6]);
}

}  // namespace

extern "C" int pcd_point_head_assign_targets_full(const float *point_coords, int num_points, const float *gt_boxes, int batch,
                                                  int n_boxes, float extra_x, float extra_y, float extra_z, int num_class,
                                                  const float *mean_size, int num_mean, long long *point_cls_labels,
                                                  float *point_box_labels, float *point_part_labels, int *num_pos, void *stream) {
    PCD_ENTER();
    if (num_points < 0 || batch < 1 || n_boxes < 0 || num_class < 1 || num_mean < 0 || !num_pos) return PCD_ERR_INVALID_ARG;
    if (num_points > 0 && (!point_coords || !point_cls_labels)) return PCD_ERR_INVALID_ARG;
    if (n_boxes > 0 && !gt_boxes) return PCD_ERR_INVALID_ARG;
    if ((num_mean > 0) != (mean_size != nullptr) || ((uintptr_t)point_box_labels & 15)) return PCD_ERR_INVALID_ARG;
    if (num_mean > PH_MAX_MEAN) return PCD_ERR_UNSUPPORTED;
    const bool want_rows = point_box_labels || point_part_labels;            // (the widest row indexed: [N][8] or [N][4])
    if ((long long)num_points * (want_rows ? 8 : 4) >= (1ll << 31) || (long long)batch * n_boxes * 8 >= (1ll << 31))
        return PCD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    ph_clear_kernel<<<1, 1, 0, st>>>(num_pos);
    if (num_points > 0 && !want_rows) {
        ph_assign_kernel<PhNoRows><<<pcd_div_up(num_points, 256), 256, 0, st>>>(point_coords, num_points, gt_boxes, batch, n_boxes,
                                                                                extra_x, extra_y, extra_z, num_class,
                                                                                point_cls_labels, num_pos, PhNoRows{});
    } else if (num_points > 0) {
        PhRows rows;
        rows.box_labels = point_box_labels;
        rows.part_labels = point_part_labels;
        rows.mean_size = mean_size;
        rows.num_mean = num_mean;
        ph_assign_kernel<PhRows><<<pcd_div_up(num_points, 256), 256, 0, st>>>(point_coords, num_points, gt_boxes, batch, n_boxes,
                                                                              extra_x, extra_y, extra_z, num_class,
                                                                              point_cls_labels, num_pos, rows);
    }
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_point_head_loss_workspace_bytes(int num_points) {
    if (num_points < 0) return 0;
    return ws_piece((size_t)(pcd_div_up(num_points, 256) + 1) * 3, sizeof(float));
}

static bool ph_loss_args_ok(const void *logits, int dtype, long long row_stride, const long long *labels, const int *num_pos,
                            int num_points, int num_class) {
    return logits && labels && num_pos && (dtype == PCD_F32 || dtype == PCD_BF16) && num_points >= 1 && num_class >= 1 &&
           row_stride >= num_class;
}

extern "C" int pcd_point_head_loss_forward(const void *logits, int dtype, long long row_stride, const long long *point_cls_labels,
                                           const int *num_pos, int num_points, int num_class, float cls_weight, float *out,
                                           void *workspace, size_t workspace_bytes, void *stream) {
    PCD_ENTER();
    if (!ph_loss_args_ok(logits, dtype, row_stride, point_cls_labels, num_pos, num_points, num_class) || !out)
        return PCD_ERR_INVALID_ARG;
    WsCarver ws(workspace, workspace_bytes);
    const int blocks = pcd_div_up(num_points, 256);
    float *partials = ws.take<float>((size_t)(blocks + 1) * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    ph_loss_kernel<false><<<blocks, 256, 0, st>>>(logits, nullptr, dtype, row_stride, point_cls_labels, num_pos, num_points,
                                                  num_class, cls_weight, nullptr, partials);
    // the anchor heads' ordered finish: sum * 1 * cls_w, no other terms
    anc_loss_finish_kernel<<<1, 256, 0, st>>>(partials, blocks, cls_weight, 0.f, 0.f, 1.f, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_point_head_loss_backward(const void *logits, void *d_logits, int dtype, long long row_stride,
                                            const long long *point_cls_labels, const int *num_pos, int num_points, int num_class,
                                            float cls_weight, const float *grad_out, void *stream) {
    PCD_ENTER();
    if (!ph_loss_args_ok(logits, dtype, row_stride, point_cls_labels, num_pos, num_points, num_class) || !d_logits || !grad_out)
        return PCD_ERR_INVALID_ARG;
    ph_loss_kernel<true><<<pcd_div_up(num_points, 256), 256, 0, (hipStream_t)stream>>>(
        logits, d_logits, dtype, row_stride, point_cls_labels, num_pos, num_points, num_class, cls_weight, grad_out, nullptr);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" size_t pcd_point_head_full_loss_workspace_bytes(int num_points) {
    return pcd_point_head_loss_workspace_bytes(num_points);
}

// the argument rules both directions share: a box / part prediction comes with its labels (and the box term with its code
// weights); a branch that is absent has NULL everywhere
static bool ph_full_loss_args_ok(const void *cls, long long cls_stride, const void *box, long long box_stride, const void *part,
                                 long long part_stride, int dtype, const long long *labels, const float *box_labels,
                                 const float *part_labels, const int *num_pos, const float *code_weights, int num_points,
                                 int num_class) {
    if (!ph_loss_args_ok(cls, dtype, cls_stride, labels, num_pos, num_points, num_class)) return false;
    if (box && (!box_labels || !code_weights || box_stride < 8)) return false;
    if (part && (!part_labels || part_stride < 3)) return false;
    return true;
}

extern "C" int pcd_point_head_full_loss_forward(const void *cls_preds, long long cls_stride, const void *box_preds,
                                                long long box_stride, const void *part_preds, long long part_stride, int dtype,
                                                const long long *point_cls_labels, const float *point_box_labels,
                                                const float *point_part_labels, const int *num_pos, const float *code_weights,
                                                int num_points, int num_class, float cls_weight, float box_weight,
                                                float part_weight, float *out, void *workspace, size_t workspace_bytes,
                                                void *stream) {
    PCD_ENTER();
    if (!ph_full_loss_args_ok(cls_preds, cls_stride, box_preds, box_stride, part_preds, part_stride, dtype, point_cls_labels,
                              point_box_labels, point_part_labels, num_pos, code_weights, num_points, num_class) || !out)
        return PCD_ERR_INVALID_ARG;
    WsCarver ws(workspace, workspace_bytes);
    const int blocks = pcd_div_up(num_points, 256);
    float *partials = ws.take<float>((size_t)(blocks + 1) * 3);
    if (!ws.ok) return PCD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    PhPreds q = {cls_preds, box_preds, part_preds, nullptr, nullptr, nullptr, cls_stride, box_stride, part_stride, dtype};
    ph_full_loss_kernel<false><<<blocks, 256, 0, st>>>(q, point_cls_labels, point_box_labels, point_part_labels, num_pos,
                                                       code_weights, num_points, num_class, cls_weight, box_weight, part_weight,
                                                       nullptr, partials);
    // the anchor heads' ordered finish: out = cls + (box + part), cls, box, part; an absent term's slot holds zeros
    anc_loss_finish_kernel<<<1, 256, 0, st>>>(partials, blocks, cls_weight, box_preds ? box_weight : 0.f,
                                              part_preds ? part_weight : 0.f, 1.f, out);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_point_head_full_loss_backward(const void *cls_preds, void *d_cls, long long cls_stride, const void *box_preds,
                                                 void *d_box, long long box_stride, const void *part_preds, void *d_part,
                                                 long long part_stride, int dtype, const long long *point_cls_labels,
                                                 const float *point_box_labels, const float *point_part_labels,
                                                 const int *num_pos, const float *code_weights, int num_points, int num_class,
                                                 float cls_weight, float box_weight, float part_weight, const float *grad_out,
                                                 void *stream) {
    PCD_ENTER();
    if (!ph_full_loss_args_ok(cls_preds, cls_stride, box_preds, box_stride, part_preds, part_stride, dtype, point_cls_labels,
                              point_box_labels, point_part_labels, num_pos, code_weights, num_points, num_class) ||
        !grad_out || !d_cls || (box_preds && !d_box) || (part_preds && !d_part))
        return PCD_ERR_INVALID_ARG;
    PhPreds q = {cls_preds, box_preds, part_preds, d_cls, d_box, d_part, cls_stride, box_stride, part_stride, dtype};
    ph_full_loss_kernel<true><<<pcd_div_up(num_points, 256), 256, 0, (hipStream_t)stream>>>(
        q, point_cls_labels, point_box_labels, point_part_labels, num_pos, code_weights, num_points, num_class, cls_weight,
        box_weight, part_weight, grad_out, nullptr);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}

extern "C" int pcd_point_head_decode(const void *cls_preds, long long cls_stride, int num_class, const long long *pred_classes,
                                     const void *box_encodings, long long enc_stride, int dtype, const float *points,
                                     long long point_stride, const float *mean_size, int num_mean, int num_points, float *boxes,
                                     void *stream) {
    PCD_ENTER();
    if (num_points < 0 || num_mean < 0 || (num_mean > 0) != (mean_size != nullptr)) return PCD_ERR_INVALID_ARG;
    if (dtype != PCD_F32 && dtype != PCD_BF16) return PCD_ERR_INVALID_ARG;
    if (num_mean > PH_MAX_MEAN || (mean_size && !pred_classes && num_class > num_mean)) return PCD_ERR_UNSUPPORTED;
    if (num_points == 0) return PCD_OK;
    if (!box_encodings || !points || !boxes || enc_stride < 8 || point_stride < 3) return PCD_ERR_INVALID_ARG;
    if (mean_size && !pred_classes && (!cls_preds || num_class < 1 || cls_stride < num_class)) return PCD_ERR_INVALID_ARG;
    if ((long long)num_points * 8 >= (1ll << 31)) return PCD_ERR_UNSUPPORTED;
    ph_decode_kernel<<<pcd_div_up(num_points, 256), 256, 0, (hipStream_t)stream>>>(
        cls_preds, cls_stride, num_class, pred_classes, box_encodings, enc_stride, dtype, points, point_stride, mean_size,
        num_mean, num_points, boxes);
    PCD_RETURN_IF_LAUNCH_FAILED();
    return PCD_OK;
}
