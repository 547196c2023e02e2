// Head tracking (include/bas.h "head tracking"): a world-frame direction and the listener's head
// orientation -> the head-relative (elevation, azimuth) the render consumes.  Shared by bas_head_relative_f64
// (bas_head.hip) and the fused pack bas_stream_batch_pack_head_f32 (bas_stream_batch.hip), which must give the same bits:
// floating-point contraction is off inside the function, so every caller evaluates the same roundings whatever the
// compiler would fuse around it, and the transcendental functions are the same device library calls in both.
#pragma once
#include <hip/hip_runtime.h>

// Direction of (el, az): d = (-sin az cos el, cos az cos el, sin el) (+y front, +z up, +x the listener's right; azimuth
// grows to the left).  q = (w, x, y, z) rotates head coordinates into world ones, d_world = R(q) d_head, so
// d_head = R(q)^T d_world with R the rotation matrix of q / |q|.  q is first negated when w < 0.  A pure yaw (x == y == 0
// after that) passes the elevation through bit for bit and subtracts 2 atan2(z, w) from the azimuth (nothing at all when
// z == 0: the identity changes neither angle, not even the sign of a zero).  Otherwise el_h = atan2(z_h, hypot(x_h, y_h)),
// az_h = atan2(-x_h, y_h), not wrapped (the a3 step takes the azimuth mod 2 pi).  The host statement is
// sphere.head_relative_angles; its expressions are the same, in the same order.
__device__ __forceinline__ void bas_head_relative(double w, double x, double y, double z, double el, double az,
                                                  double &el_h, double &az_h) {
#pragma clang fp contract(off)
    if (w < 0.0) {
        w = -w; x = -x; y = -y; z = -z;
    }
    if (x == 0.0 && y == 0.0) {
        el_h = el;
        az_h = z == 0.0 ? az : az - 2.0 * atan2(z, w);
        return;
    }
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w = w / n; x = x / n; y = y / n; z = z / n;
    double se, ce, sa, ca;
    sincos(el, &se, &ce);
    sincos(az, &sa, &ca);
    const double dx = -sa * ce, dy = ca * ce, dz = se;
    // R^T d: the columns of R
    const double xh = (1.0 - 2.0 * (y * y + z * z)) * dx + 2.0 * (x * y + w * z) * dy + 2.0 * (x * z - w * y) * dz;
    const double yh = 2.0 * (x * y - w * z) * dx + (1.0 - 2.0 * (x * x + z * z)) * dy + 2.0 * (y * z + w * x) * dz;
    const double zh = 2.0 * (x * z + w * y) * dx + 2.0 * (y * z - w * x) * dy + (1.0 - 2.0 * (x * x + y * y)) * dz;
    el_h = atan2(zh, hypot(xh, yh));
    az_h = atan2(-xh, yh);
}
