// Point-in-box geometry of the reference's roiaware_pool3d package, shared by the device kernels and the host entry
// point of roiaware.hip (the way iou3d_geom.h is shared).  The arithmetic is the reference's, step by step
// (roiaware_pool3d_kernel.cu:16-36, roiaware_pool3d.cpp:121-140):
//   * the z test `fabsf(z - cz) > dz / 2` runs first and rejects;
//   * cos / sin of -heading in float, local = shift_x * cos + shift_y * (-sin), shift_x * sin + shift_y * cos (two
//     products and one sum each, not fused: the file is compiled with -ffp-contract=off);
//   * the xy comparison in DOUBLE: (double)fabs(local) < (double)d / 2.0 + (double)(float)MARGIN.
// A box is prepared once (one sincos, the two double thresholds); the test itself is a few multiplies per pair.
#pragma once
#include <math.h>

#ifndef __host__
#define __host__
#define __device__
#endif

#define RA_MARGIN_DEVICE 1e-5f   // roiaware_pool3d_kernel.cu:27
#define RA_MARGIN_HOST 1e-2f     // roiaware_pool3d.cpp:131
#define RA_CHUNK 128             // boxes a workgroup stages in LDS per pass (roiaware.hip, pointhead.hip)

struct RaBox {
    float cx, cy, cz, hz, cosa, sina;
    double tx, ty;               // dx / 2.0 + MARGIN, dy / 2.0 + MARGIN
};

// thresholds of a box with extents (dx, dy, dz)
__host__ __device__ inline void ra_extents(RaBox &b, float dx, float dy, float dz, float margin) {
    b.hz = dz / 2.0f;                                        // exact: the reference's dz / 2.0 as a float
    b.tx = (double)dx / 2.0 + (double)margin;
    b.ty = (double)dy / 2.0 + (double)margin;
}

__host__ __device__ inline RaBox ra_prepare(const float *box, float margin) {
    RaBox b;
    b.cx = box[0];
    b.cy = box[1];
    b.cz = box[2];
    const float rz = box[6];
    b.cosa = cosf(-rz);
    b.sina = sinf(-rz);
    ra_extents(b, box[3], box[4], box[5], margin);
    return b;
}

__host__ __device__ inline bool ra_z_inside(float z, float cz, float hz) { return !(fabsf(z - cz) > hz); }

__host__ __device__ inline void ra_local(const RaBox &b, float x, float y, float &lx, float &ly) {
    const float sx = x - b.cx, sy = y - b.cy;
    lx = sx * b.cosa + sy * (-b.sina);
    ly = sx * b.sina + sy * b.cosa;
}

__host__ __device__ inline bool ra_xy_inside(float lx, float ly, double tx, double ty) {
    return ((double)fabsf(lx) < tx) && ((double)fabsf(ly) < ty);
}

// check_pt_in_box3d: local_x / local_y are only written when the z test passes (as in the reference)
__host__ __device__ inline bool ra_point_in_box(const RaBox &b, float x, float y, float z, float &lx, float &ly) {
    if (!ra_z_inside(z, b.cz, b.hz)) return false;
    ra_local(b, x, y, lx, ly);
    return ra_xy_inside(lx, ly, b.tx, b.ty);
}

#ifdef __HIPCC__
// The voxel of a point inside a RoI along one axis (RoI-aware pooling, roiaware.hip and parta2.hip):
// int((local + d / 2) / res) clamped to [0, out - 1]   (roiaware_pool3d_kernel.cu:60-70).  nan and every negative
// quotient give 0: the reference's unsigned compare would send a quotient <= -1 to out - 1, which local + d / 2 >=
// -MARGIN makes unreachable for a box wider than 1e-5 m per voxel
__device__ __forceinline__ int ra_voxel_index(float local, float d, float res, int out) {
    const float q = __fdiv_rn(local + d / 2.f, res);
    if (!(q >= 1.f)) return 0;
    return q < (float)out ? (int)q : out - 1;
}
#endif
