// The cuboid interior test shared by targets.hip (dense target assignment) and dbsample.hip (the object-database builder).
//
// Reference: cuboids_to_vertices / compute_interior_points_mask (math/polytope.py:14-107).  Numerics follow the reference: box
// vertices in fp32 through the yaw-only quaternion, the three slab tests in fp64.  `cub` is a row of the (m,10) fp64 cuboid table
// [x, y, z, l, w, h, yaw, ...] of rv_assign_targets.
#pragma once
#include "common.h"

namespace {

struct BoxPlanes {
    double uvw[3][3];
    double lo[3], hi[3];  // the slab [min(d_ref,d_cor), max(d_ref,d_cor)] of each axis
};

__device__ void make_planes(const double* cub, BoxPlanes* bp) {
    const float cx = (float)cub[0], cy = (float)cub[1], cz = (float)cub[2];
    const float hl = (float)cub[3] / 2.0f, hw = (float)cub[4] / 2.0f, hh = (float)cub[5] / 2.0f;
    const float half = (float)cub[6] * 0.5f;
    float qw = cosf(half), qz = sinf(half);
    const float nrm = sqrtf(qw * qw + qz * qz);
    qw /= nrm;
    qz /= nrm;
    const float r00 = 1.f - 2.f * (qz * qz), r01 = 2.f * (0.f - qw * qz), r10 = 2.f * (qw * qz), r11 = r00;
    // unit vertices: 1 (+,-,+)  2 (+,-,-)  3 (+,+,-)  6 (-,-,-)   (math/polytope.py:79-91)
    const float ux[4] = {+1.f, +1.f, +1.f, -1.f};
    const float uy[4] = {-1.f, -1.f, +1.f, -1.f};
    const float uz[4] = {+1.f, -1.f, -1.f, -1.f};
    double v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ox = hl * ux[k], oy = hw * uy[k], oz = hh * uz[k];
        v[k][0] = (double)(ox * r00 + oy * r01 + cx);
        v[k][1] = (double)(ox * r10 + oy * r11 + cy);
        v[k][2] = (double)(oz + cz);
    }
    // reference vertex = 2; corners = vertices [6, 3, 1]
    const int corner[3] = {3, 2, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double dref = 0.0, dcor = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double u = v[1][j] - v[corner[a]][j];
            bp->uvw[a][j] = u;
            dref += u * v[1][j];
            dcor += u * v[corner[a]][j];
        }
        bp->lo[a] = dref < dcor ? dref : dcor;
        bp->hi[a] = dref < dcor ? dcor : dref;
    }
}

__device__ __forceinline__ bool inside(const BoxPlanes& bp, double x, double y, double z) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double d = bp.uvw[a][0] * x + bp.uvw[a][1] * y + bp.uvw[a][2] * z;
        if (!(bp.lo[a] <= d && d <= bp.hi[a])) return false;
    }
    return true;
}

}  // namespace
