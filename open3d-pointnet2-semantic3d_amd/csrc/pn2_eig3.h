// pn2_eig3.h -- the principal axes of a symmetric 3 x 3 matrix by the rules of include/pn2_abi.h ("Object description", AXES), in
// one copy: pn2_describe.hip (per cluster) and pn2_neighbors.hip (per point).  Float64 in the written association, without
// contraction; sqrt and / are correctly rounded: the result is a function of the six entries alone.
#pragma once
#include <hip/hip_runtime.h>

// one Jacobi rotation on the pair (p, r), k the third index: the rules of include/pn2_abi.h, in their written association
__device__ __forceinline__ void jacobi_rotate(double& app, double& arr, double& apr, double& akp, double& akr, double* vp,
                                              double* vr) {
    if (apr == 0.0) return;
    const double theta = (arr - app) / (2.0 * apr);
    const double sigma = theta >= 0.0 ? 1.0 : -1.0;
    const double t = sigma / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
    const double s = t * c;
    app -= t * apr;
    arr += t * apr;
    apr = 0.0;
    const double nkp = c * akp - s * akr, nkr = s * akp + c * akr;
    akp = nkp;
    akr = nkr;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double np = c * vp[i] - s * vr[i], nr = s * vp[i] + c * vr[i];
        vp[i] = np;
        vr[i] = nr;
    }
}

// negate v when its component of largest magnitude, the first among equals, is negative
__device__ __forceinline__ void fix_sign(double* v) {
    int at = 0;
    if (__builtin_fabs(v[1]) > __builtin_fabs(v[at])) at = 1;
    if (__builtin_fabs(v[2]) > __builtin_fabs(v[at])) at = 2;
    if (v[at] < 0.0) {
        v[0] = -v[0];
        v[1] = -v[1];
        v[2] = -v[2];
    }
}

// the upper triangle of A (taken by value: it is rotated away) -> lam descending, a0 = e0 and a1 = e1 sign-fixed, e2 = e0 x e1:
// eight cyclic sweeps from V = identity, the stable sort of the three eigenpairs, the cross product
__device__ __forceinline__ void eig3_axes(double a00, double a01, double a02, double a11, double a12, double a22, double* lam,
                                          double* e0, double* e1, double* e2) {
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};  // the COLUMNS of V
    for (int sweep = 0; sweep < 8; ++sweep) {
        jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);  // (0,1), k = 2
        jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);  // (0,2), k = 1
        jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);  // (1,2), k = 0
    }
    // a stable bubble sort of three, descending: a swap only on a strict "less"
    double dg[3] = {a00, a11, a22};
    double col[3][3];
    for (int i = 0; i < 3; ++i) { col[0][i] = v0[i]; col[1][i] = v1[i]; col[2][i] = v2[i]; }
    for (int pass = 0; pass < 2; ++pass)
        for (int j = 0; j < 2 - pass; ++j)
            if (dg[j] < dg[j + 1]) {
                const double t = dg[j]; dg[j] = dg[j + 1]; dg[j + 1] = t;
                for (int i = 0; i < 3; ++i) { const double u = col[j][i]; col[j][i] = col[j + 1][i]; col[j + 1][i] = u; }
            }
    for (int i = 0; i < 3; ++i) { lam[i] = dg[i]; e0[i] = col[0][i]; e1[i] = col[1][i]; }
    fix_sign(e0);
    fix_sign(e1);
    e2[0] = e0[1] * e1[2] - e0[2] * e1[1];
    e2[1] = e0[2] * e1[0] - e0[0] * e1[2];
    e2[2] = e0[0] * e1[1] - e0[1] * e1[0];
}
