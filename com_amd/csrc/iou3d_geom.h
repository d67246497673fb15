// Rotated BEV overlap / IoU geometry of the reference's iou3d_nms_kernel.cu:14-234,312-324, shared by the NMS kernels of
// iou3d.hip (pcd_nms_bev) and the batched NMS of postproc.hip: one source, so both give the same bits for the same boxes.
// Arithmetic follows the reference's float formulas step by step (see iou3d.hip).
#pragma once
#include "common.h"

namespace {

constexpr float IOU_EPS = 1e-8f;        // iou3d_nms_kernel.cu:14

// (the geometry is __host__ __device__: pcd_boxes_iou_bev_host in iou3d.hip runs the SAME code on the host, where cosf / sinf /
//  atan2f are the C library's -- the functions the reference's iou3d_cpu.cpp calls)
struct P2 {
    float x, y;
};
__host__ __device__ __forceinline__ P2 mk(float x, float y) { P2 p; p.x = x; p.y = y; return p; }
__host__ __device__ __forceinline__ float cross2(const P2 &a, const P2 &b) { return a.x * b.y - a.y * b.x; }
// (p1 - p0) x (p2 - p0)
__host__ __device__ __forceinline__ float cross3(const P2 &p1, const P2 &p2, const P2 &p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// bounding boxes of the two segments overlap (iou3d_nms_kernel.cu:43-49)
__host__ __device__ __forceinline__ bool seg_boxes_touch(const P2 &p1, const P2 &p2, const P2 &q1, const P2 &q2) {
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// point inside the rotated rectangle, with the reference's 1e-2 margin (iou3d_nms_kernel.cu:51-61)
__host__ __device__ __forceinline__ bool in_box2d(const float *box, const P2 &p) {
    const float MARGIN = 1e-2f;
    const float cx = box[0], cy = box[1];
    const float c = cosf(-box[6]), s = sinf(-box[6]);
    const float rx = (p.x - cx) * c + (p.y - cy) * (-s);
    const float ry = (p.x - cx) * s + (p.y - cy) * c;
    return fabsf(rx) < box[3] / 2 + MARGIN && fabsf(ry) < box[4] / 2 + MARGIN;
}

// proper intersection of segments p0-p1 and q0-q1 (iou3d_nms_kernel.cu:63-92)
__host__ __device__ __forceinline__ bool seg_intersection(const P2 &p1, const P2 &p0, const P2 &q1, const P2 &q0, P2 &ans) {
    if (!seg_boxes_touch(p0, p1, q0, q1)) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > IOU_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__host__ __device__ __forceinline__ void corners_of(const float *box, P2 (&c)[5]) {
    const float hx = box[3] / 2, hy = box[4] / 2;
    const float x1 = box[0] - hx, y1 = box[1] - hy, x2 = box[0] + hx, y2 = box[1] + hy;
    const float ca = cosf(box[6]), sa = sinf(box[6]);
    const float px[4] = {x1, x2, x2, x1}, py[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // rotate around the centre (iou3d_nms_kernel.cu:94-98)
        c[k].x = (px[k] - box[0]) * ca + (py[k] - box[1]) * (-sa) + box[0];
        c[k].y = (px[k] - box[0]) * sa + (py[k] - box[1]) * ca + box[1];
    }
    c[4] = c[0];
}

// area of the intersection polygon of two rotated rectangles (iou3d_nms_kernel.cu:104-223)
__host__ __device__ inline float overlap_bev(const float *a, const float *b) {
    P2 ca[5], cb[5];
    corners_of(a, ca);
    corners_of(b, cb);
    P2 pts[16];
    P2 centre = mk(0.f, 0.f);
    int cnt = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 x;
            if (seg_intersection(ca[i + 1], ca[i], cb[j + 1], cb[j], x)) {
                centre.x += x.x;
                centre.y += x.y;
                pts[cnt++] = x;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(a, cb[k])) {
            centre.x += cb[k].x;
            centre.y += cb[k].y;
            pts[cnt++] = cb[k];
        }
        if (in_box2d(b, ca[k])) {
            centre.x += ca[k].x;
            centre.y += ca[k].y;
            pts[cnt++] = ca[k];
        }
    }
    centre.x /= cnt;      // (cnt == 0: inf / nan, never used -- the loops below do not run)
    centre.y /= cnt;
    // bubble sort by polar angle around the centroid, exactly the reference's passes (its predicate is `>` on
    // atan2 values, so ties are left in place)
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i) {
            const float ai = atan2f(pts[i].y - centre.y, pts[i].x - centre.x);
            const float an = atan2f(pts[i + 1].y - centre.y, pts[i + 1].x - centre.x);
            if (ai > an) {
                const P2 t = pts[i];
                pts[i] = pts[i + 1];
                pts[i + 1] = t;
            }
        }
    float area = 0.f;
    for (int k = 0; k < cnt - 1; ++k)
        area += cross2(mk(pts[k].x - pts[0].x, pts[k].y - pts[0].y), mk(pts[k + 1].x - pts[0].x, pts[k + 1].y - pts[0].y));
    return fabsf(area) / 2.0f;
}

__host__ __device__ __forceinline__ float iou_bev_dev(const float *a, const float *b) {     // iou3d_nms_kernel.cu:225-234
    const float sa = a[3] * a[4], sb = b[3] * b[4];
    const float so = overlap_bev(a, b);
    return so / fmaxf(sa + sb - so, IOU_EPS);
}

__device__ __forceinline__ float iou_normal_dev(const float *a, const float *b) {  // iou3d_nms_kernel.cu:312-324
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float w = fmaxf(right - left, 0.f), h = fmaxf(bottom - top, 0.f);
    const float inter = w * h;
    return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, IOU_EPS);
}

}  // namespace
