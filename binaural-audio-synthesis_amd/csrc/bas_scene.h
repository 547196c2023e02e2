// Cartesian scenes (include/bas.h "Cartesian scenes"): one source position, one shoebox image index, the
// listener's pose -> the (elevation, azimuth, gain, delay) the render consumes for that image source at one chunk
// boundary.  Binary64 throughout, floating-point contraction off inside the function (as in bas_head.h): the host
// statement scene.scene_params evaluates the same expressions in the same order, so the two differ only by the last
// places of hypot and atan2.
#pragma once
#include <hip/hip_runtime.h>

struct BasScenePoint {
    double el, az, gain, delay;
    double r, cos_theta;        // path length and emission angle's cosine (directed only)
    double qx, qy, qz;          // the image's position after steps 1 and 1b: the path's far end (screens)
};

// p: the source, l: the listener (world frame, metres).  room: L = the shoebox's size and m = the image's index per axis
// (q_a = m L_a + (m even ? p_a : L_a - p_a)); free field otherwise (q = p).  head: (w, x, y, z) rotating head coordinates
// into world ones, any non-zero norm; v_h = R(q / |q|)^T v with the matrix of bas_head.h.  Directions follow the
// reference's convention (sphere.py:51-56): +y front, +z up, +x right, azimuth to the left, not wrapped.  v == 0 exactly
// gives el = az = 0.  g = src_gain * img_gain; gain = g r_ref / max(r, r_ref); delay = r spm clamped to [dmin, dmax].
// moving: the source is heard where it was when the sound left it.  (ax, ay, az) and (bx, by, bz) are its positions one
// chunk of spc samples apart around this boundary; the image moves at u = (q(b) - q(a)) / spc per sample, and the delay d
// that solves |q - u d - l| = d / spm (a quadratic; subsonic u only, else no correction) puts it at q - u d for steps 2-6.
// directed (bas_scene_params_bands_f64 only): o = (ow, ox, oy, oz) turns the source's frame into the world frame, any
// non-zero norm; the source radiates along its local +y, f = R(o / |o|) (0, 1, 0); an image's axis is f with component a
// negated where m_a is odd; cos_theta = f . (l - q) / r for the q of steps 2-6 (r == 0: 1), r unclamped.  The other four
// results do not depend on it.
__device__ __forceinline__ BasScenePoint bas_scene_point(double px, double py, double pz, double lx, double ly, double lz,
                                                         bool moving, double ax, double ay, double az_, double bx, double by,
                                                         double bz, double spc,
                                                         bool room, double Lx, double Ly, double Lz, int mx, int my, int mz,
                                                         bool head, double w, double x, double y, double z, double sgain,
                                                         double igain, double spm, double r_ref, double dmin, double dmax,
                                                         bool directed = false, double ow = 1.0, double ox = 0.0,
                                                         double oy = 0.0, double oz = 0.0) {
#pragma clang fp contract(off)
    if (room) {
        px = (double)mx * Lx + ((mx & 1) ? Lx - px : px);
        py = (double)my * Ly + ((my & 1) ? Ly - py : py);
        pz = (double)mz * Lz + ((mz & 1) ? Lz - pz : pz);
    }
    if (moving) {
        if (room) {                                        // (the images of both ends: the mirror turns the velocity too)
            ax = (double)mx * Lx + ((mx & 1) ? Lx - ax : ax); bx = (double)mx * Lx + ((mx & 1) ? Lx - bx : bx);
            ay = (double)my * Ly + ((my & 1) ? Ly - ay : ay); by = (double)my * Ly + ((my & 1) ? Ly - by : by);
            az_ = (double)mz * Lz + ((mz & 1) ? Lz - az_ : az_); bz = (double)mz * Lz + ((mz & 1) ? Lz - bz : bz);
        }
        const double ux = (bx - ax) / spc, uy = (by - ay) / spc, uz = (bz - az_) / spc;
        const double wx = px - lx, wy = py - ly, wz = pz - lz;
        const double A = 1.0 / (spm * spm) - (ux * ux + uy * uy + uz * uz);
        if (A > 0.0) {
            const double wu = wx * ux + wy * uy + wz * uz;
            const double d = (sqrt(wu * wu + A * (wx * wx + wy * wy + wz * wz)) - wu) / A;
            px = px - ux * d; py = py - uy * d; pz = pz - uz * d;
        }
    }
    double vx = px - lx, vy = py - ly, vz = pz - lz;
    const double r = sqrt(vx * vx + vy * vy + vz * vz);
    const bool at_listener = vx == 0.0 && vy == 0.0 && vz == 0.0;
    if (head) {
        const double n = sqrt(w * w + x * x + y * y + z * z);
        w = w / n; x = x / n; y = y / n; z = z / n;
        // R^T v: the columns of R
        const double xh = (1.0 - 2.0 * (y * y + z * z)) * vx + 2.0 * (x * y + w * z) * vy + 2.0 * (x * z - w * y) * vz;
        const double yh = 2.0 * (x * y - w * z) * vx + (1.0 - 2.0 * (x * x + z * z)) * vy + 2.0 * (y * z + w * x) * vz;
        const double zh = 2.0 * (x * z + w * y) * vx + 2.0 * (y * z - w * x) * vy + (1.0 - 2.0 * (x * x + y * y)) * vz;
        vx = xh; vy = yh; vz = zh;
    }
    BasScenePoint o;
    o.el = at_listener ? 0.0 : atan2(vz, hypot(vx, vy));
    o.az = at_listener ? 0.0 : atan2(-vx, vy);
    o.gain = sgain * igain * r_ref / fmax(r, r_ref);
    o.delay = fmax(fmin(r * spm, dmax), dmin);
    o.r = r;
    o.qx = px; o.qy = py; o.qz = pz;
    o.cos_theta = 1.0;
    if (directed) {
        const double n = sqrt(ow * ow + ox * ox + oy * oy + oz * oz);
        ow = ow / n; ox = ox / n; oy = oy / n; oz = oz / n;
        double fx = 2.0 * (ox * oy - ow * oz), fy = 1.0 - 2.0 * (ox * ox + oz * oz), fz = 2.0 * (oy * oz + ow * ox);
        if (room) {
            if (mx & 1) fx = -fx;
            if (my & 1) fy = -fy;
            if (mz & 1) fz = -fz;
        }
        // (v of step 2, before the head turned it: px - lx is q - l, and the emission runs the other way)
        const double dot = fx * (px - lx) + fy * (py - ly) + fz * (pz - lz);
        o.cos_theta = r == 0.0 ? 1.0 : -dot / r;
    }
    return o;
}
