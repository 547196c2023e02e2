// Ambisonic beds (include/bas.h "ambisonic beds"): the limits and tile of bas_ambi.hip, and the device
// functions its kernels share - the real spherical harmonics (N3D, ACN order, no Condon-Shortley phase) and the head's
// rotation R(q)^T of "head tracking".  Floating-point contraction is off inside them: every caller evaluates the same
// roundings whatever the compiler would fuse around them.
#pragma once
#include <hip/hip_runtime.h>

#define AMBI_MAX_ORDER 3
#define AMBI_MAX_C 16                   // (AMBI_MAX_ORDER + 1)^2
#define AMBI_MAX_V 64
#define AMBI_MAX_J 64
#define AMBI_THREADS 256                // one workgroup per (group, boundary) of bas_ambi_matrices_f32

#define MM_THREADS 256
#define MM_TILE 1024                    // outputs of one workgroup pass of bas_matrix_mix_f32: four per lane
#define MM_FILL 512                     // workgroups the speaker rows are dealt to (blockIdx.z) where tiles x groups < 256
#define MM_LDS_FLOATS 8192              // matrices a tile can hold in LDS: MM_LDS_FLOATS / (V CP) boundaries (>= 8)

// The encoder (include/bas.h "ambisonic encoder")
#define ENCODE_BLOCK 32                 // sources of one first-level chain of bas_ambi_encode_f32 (part of the definition)
#define ENC_MAX_SRC 65536
#define ENC_THREADS 256
#define ENC_TILE 1024                   // outputs of one workgroup pass: four per lane
#define ENC_FILL 512                    // below ENC_FILL / 2 workgroups the channels are dealt in slices of four
#define ENC_LDS_FLOATS 8192             // the banks of one slab of sources: n_sets x slab x (channels of the slice)
#define ENC_MAX_SLAB 512                // sources of one LDS stage at most (a longer stage saves nothing)
#define ENC_STATIC_SLICE 16             // channels one workgroup accumulates: 16 x 4 block sums + 16 x 4 totals = 128 registers
#define ENC_BOUNDARY_SLICE 8            // .. with two banks: 8 x 4 x 2 + 8 x 4 x 2

// Y_0 .. Y_{C-1} of the unit vector d (project frame: +y front, +x right, +z up) in (x, y, z) = (d_y, -d_x, d_z).  The
// constants are the correctly rounded binary64 square roots.
__device__ __forceinline__ void bas_sh_n3d(double dx, double dy, double dz, int order, double *Y) {
#pragma clang fp contract(off)
    const double x = dy, y = -dx, z = dz;
    Y[0] = 1.0;
    Y[1] = 1.7320508075688772 * y;
    Y[2] = 1.7320508075688772 * z;
    Y[3] = 1.7320508075688772 * x;
    if (order >= 2) {
        Y[4] = 3.872983346207417 * (x * y);
        Y[5] = 3.872983346207417 * (y * z);
        Y[6] = 1.118033988749895 * (3.0 * (z * z) - 1.0);
        Y[7] = 3.872983346207417 * (x * z);
        Y[8] = 1.9364916731037085 * (x * x - y * y);
    }
    if (order >= 3) {
        Y[9] = 2.091650066335189 * (y * (3.0 * (x * x) - y * y));
        Y[10] = 10.246950765959598 * ((x * y) * z);
        Y[11] = 1.620185174601965 * (y * (5.0 * (z * z) - 1.0));
        Y[12] = 1.3228756555322954 * (z * (5.0 * (z * z) - 3.0));
        Y[13] = 1.620185174601965 * (x * (5.0 * (z * z) - 1.0));
        Y[14] = 5.123475382979799 * (z * (x * x - y * y));
        Y[15] = 2.091650066335189 * (x * (x * x - 3.0 * (y * y)));
    }
}

// q = (w, x, y, z) as bas_head_relative takes it: negated when w < 0.  True when x == y == z == 0 after that (the identity,
// a zero quaternion included); otherwise q is normalised in place.
__device__ __forceinline__ bool bas_ambi_unit_head(double &w, double &x, double &y, double &z) {
#pragma clang fp contract(off)
    if (w < 0.0) {
        w = -w; x = -x; y = -y; z = -z;
    }
    if (x == 0.0 && y == 0.0 && z == 0.0) return true;
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w = w / n; x = x / n; y = y / n; z = z / n;
    return false;
}

// R(q)^T s for a unit q: the columns of R, the expressions of bas_head_relative.
__device__ __forceinline__ void bas_ambi_rotate_t(double w, double x, double y, double z, double sx, double sy, double sz,
                                                  double &hx, double &hy, double &hz) {
#pragma clang fp contract(off)
    hx = (1.0 - 2.0 * (y * y + z * z)) * sx + 2.0 * (x * y + w * z) * sy + 2.0 * (x * z - w * y) * sz;
    hy = 2.0 * (x * y - w * z) * sx + (1.0 - 2.0 * (x * x + z * z)) * sy + 2.0 * (y * z + w * x) * sz;
    hz = 2.0 * (x * z + w * y) * sx + 2.0 * (y * z - w * x) * sy + (1.0 - 2.0 * (x * x + y * y)) * sz;
}
