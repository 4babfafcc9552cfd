// gs_xform_math.hip -- gs_xform_compose's mathematics (gs_abi.h "splat transforms"): the rotation matrix, the 3x4 similarity and the
// SH band matrices D_1..D_3 of a rotation, in double, every output rounded to f32 once.  Plain C++: no HIP call, no context.
//
// The reference has no counterpart (a viewer never rotates its coefficients); what fixes D_l is its own compute_color_from_sh
// (process_gaussians.wgsl:240-280): with B_l(d) the vector of that function's band-l terms, a splat rotated by R and seen from d
// must show what the original showed from R^T d, for every coefficient vector c:  B_l(d) . (D_l c) = B_l(R^T d) . c, i.e.
//     D_l^T B_l(d) = B_l(R^T d)   for every unit d.
// Band l spans a (2l+1)-dimensional rotation-invariant space, so the identity on enough directions fixes D_l.  It is solved here over
// K = 24 fixed directions (a golden-angle spiral: the Gram matrix Y Y^T of every band has a condition number below 2) through the
// normal equations  (Y Y^T) D_l = Y Y'^T,  Y = [B_l(d_k)], Y' = [B_l(R^T d_k)] -- no recurrence, no table of signs to get wrong: the
// basis function below is the only place where the reference's order and signs are written down.
#include "gs_xform_math.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <utility>

static const double kC1 = 0.4886025119029199;
static const double kC2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
static const double kC3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                              -0.4570457994644658, 1.445305721320277,  -0.5900435899266435};

void gs_xform_sh_basis(int l, const double d[3], double* o) {
    const double x = d[0], y = d[1], z = d[2];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
    if (l == 1) {
        o[0] = -kC1 * y; o[1] = kC1 * z; o[2] = -kC1 * x;
    } else if (l == 2) {
        o[0] = kC2[0] * xy; o[1] = kC2[1] * yz; o[2] = kC2[2] * (2.0 * zz - xx - yy); o[3] = kC2[3] * xz; o[4] = kC2[4] * (xx - yy);
    } else {
        o[0] = kC3[0] * y * (3.0 * xx - yy);
        o[1] = kC3[1] * xy * z;
        o[2] = kC3[2] * y * (4.0 * zz - xx - yy);
        o[3] = kC3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
        o[4] = kC3[4] * x * (4.0 * zz - xx - yy);
        o[5] = kC3[5] * z * (xx - yy);
        o[6] = kC3[6] * x * (xx - 3.0 * yy);
    }
}

static const int kDirs = 24;
static void direction(int k, double d[3]) { // golden-angle spiral over the sphere
    const double z = 1.0 - 2.0 * (k + 0.5) / kDirs, r = std::sqrt(1.0 - z * z), ph = k * 2.399963229728653;
    d[0] = r * std::cos(ph); d[1] = r * std::sin(ph); d[2] = z;
}

// A X = B for n <= 7, A symmetric positive definite (n x n), B n x n, all row-major with stride 7; partial pivoting all the same.
static bool solve(int n, double A[7][7], double B[7][7]) {
    for (int c = 0; c < n; ++c) {
        int p = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
        if (!(std::fabs(A[p][c]) > 1e-12)) return false;
        if (p != c)
            for (int k = 0; k < n; ++k) { std::swap(A[p][k], A[c][k]); std::swap(B[p][k], B[c][k]); }
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            if (f == 0.0) continue;
            for (int k = 0; k < n; ++k) { A[r][k] -= f * A[c][k]; B[r][k] -= f * B[c][k]; }
        }
    }
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < n; ++k) B[r][k] /= A[r][r];
    return true;
}

// D_l of the rotation R (row-major 3x3), row-major (2l+1) x (2l+1) into out, rounded once.
static bool band_matrix(int l, const double R[9], float* out) {
    const int n = 2 * l + 1;
    double G[7][7] = {}, H[7][7] = {};
    for (int k = 0; k < kDirs; ++k) {
        double d[3], e[3], y[7], yr[7];
        direction(k, d);
        for (int c = 0; c < 3; ++c) e[c] = R[0 + c] * d[0] + R[3 + c] * d[1] + R[6 + c] * d[2]; // R^T d
        gs_xform_sh_basis(l, d, y);
        gs_xform_sh_basis(l, e, yr);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) { G[i][j] += y[i] * y[j]; H[i][j] += y[i] * yr[j]; }
    }
    if (!solve(n, G, H)) return false;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double v = H[i][j];
            // what the solve leaves of an exact 0 or +-1 (a quarter turn about an axis is a signed permutation)
            if (std::fabs(v) < 1e-14) v = 0.0;
            else if (std::fabs(std::fabs(v) - 1.0) < 1e-14) v = v < 0.0 ? -1.0 : 1.0;
            out[i * n + j] = (float)v;
        }
    return true;
}

static int32_t refuse(char* err, size_t errlen, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return GS_ERR_INVALID_ARGUMENT;
}

int32_t gs_xform_compose_host(const float* rot, const float* tr, float scale, const float* pivot, gs_xform* out, char* err, size_t errlen) {
    if (!rot) return refuse(err, errlen, "gs_xform_compose: null rot_rxyz");
    if (!tr) return refuse(err, errlen, "gs_xform_compose: null translate");
    if (!out) return refuse(err, errlen, "gs_xform_compose: null out");
    double q[4], len2 = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (!std::isfinite(rot[k])) return refuse(err, errlen, "gs_xform_compose: rot_rxyz[%d] is not finite", k);
        q[k] = rot[k];
        len2 += q[k] * q[k];
    }
    if (!(len2 > 0.0)) return refuse(err, errlen, "gs_xform_compose: rot_rxyz is the zero quaternion");
    if (!std::isfinite(scale) || !(scale > 0.0f)) return refuse(err, errlen, "gs_xform_compose: scale %g is not a finite positive number", (double)scale);
    double t[3], p[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(tr[k])) return refuse(err, errlen, "gs_xform_compose: translate[%d] is not finite", k);
        if (pivot && !std::isfinite(pivot[k])) return refuse(err, errlen, "gs_xform_compose: pivot[%d] is not finite", k);
        t[k] = tr[k];
        if (pivot) p[k] = pivot[k];
    }
    const double len = std::sqrt(len2);
    for (int k = 0; k < 4; ++k) q[k] /= len;
    const double r = q[0], x = q[1], y = q[2], z = q[3];
    // the rotation compute_cov3d builds from a normalised rot (process_gaussians.wgsl:127-163), as a row-major matrix acting on columns
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z),       2.0 * (x * z + r * y),
                         2.0 * (x * y + r * z),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
                         2.0 * (x * z - r * y),       2.0 * (y * z + r * x),       1.0 - 2.0 * (x * x + y * y)};
    const double s = scale;
    gs_xform o{};
    o.struct_size = (uint32_t)sizeof(gs_xform);
    for (int k = 0; k < 4; ++k) o.q[k] = (float)q[k];
    for (int row = 0; row < 3; ++row) {
        double sRp = 0.0;
        for (int c = 0; c < 3; ++c) {
            o.m[4 * row + c] = (float)(s * R[3 * row + c]);
            sRp += s * R[3 * row + c] * p[c];
        }
        o.m[4 * row + 3] = (float)(t[row] + p[row] - sRp);
    }
    o.log_scale = (float)std::log(s);
    if (!band_matrix(1, R, o.sh1) || !band_matrix(2, R, o.sh2) || !band_matrix(3, R, o.sh3))
        return refuse(err, errlen, "gs_xform_compose: the band matrices could not be solved");
    o.flags = GS_XFORM_POSITION;
    const bool identity = std::fabs(o.q[0]) == 1.0f && o.q[1] == 0.0f && o.q[2] == 0.0f && o.q[3] == 0.0f;
    if (!identity) o.flags |= GS_XFORM_ORIENT;
    if (scale != 1.0f) o.flags |= GS_XFORM_SIZE;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(o.m[k])) return refuse(err, errlen, "gs_xform_compose: the matrix overflows f32");
    *out = o;
    return GS_OK;
}
