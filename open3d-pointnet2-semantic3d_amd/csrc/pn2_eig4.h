// pn2_eig4.h -- the eigenvectors of a symmetric 4 x 4 matrix by the rules of include/pn2_abi.h ("Rigid registration (ICP)",
// POINT-TO-POINT): pn2_eig3.h's rotation, applied to the TWO other indices of a pair.  Float64 in the written association,
// without contraction; sqrt and / are correctly rounded: the result is a function of the ten entries alone.  One user,
// pn2_icp.hip (Horn's quaternion matrix); it runs in one thread, so the arrays may live wherever the compiler puts them.
#pragma once
#include <hip/hip_runtime.h>

// one rotation on the pair (p, r) of the full symmetric A (both halves are kept); V holds the eigenvectors as COLUMNS, V[i][j]
__device__ __forceinline__ void eig4_rotate(double (&A)[4][4], double (&V)[4][4], int p, int r) {
    const double apr = A[p][r];
    if (apr == 0.0) return;
    const double theta = (A[r][r] - A[p][p]) / (2.0 * apr);
    const double sigma = theta >= 0.0 ? 1.0 : -1.0;
    const double t = sigma / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
    const double s = t * c;
    A[p][p] -= t * apr;
    A[r][r] += t * apr;
    A[p][r] = A[r][p] = 0.0;
    for (int k = 0; k < 4; ++k) {
        if (k == p || k == r) continue;
        const double nkp = c * A[k][p] - s * A[k][r], nkr = s * A[k][p] + c * A[k][r];
        A[k][p] = A[p][k] = nkp;
        A[k][r] = A[r][k] = nkr;
    }
    for (int i = 0; i < 4; ++i) {
        const double np = c * V[i][p] - s * V[i][r], nr = s * V[i][p] + c * V[i][r];
        V[i][p] = np;
        V[i][r] = nr;
    }
}

// A (rotated away) -> q = the column of V under the largest diagonal entry, the first among equals: ten cyclic sweeps over the
// pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) from V = identity
__device__ __forceinline__ void eig4_largest(double (&A)[4][4], double* q) {
    double V[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 10; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) eig4_rotate(A, V, p, r);
    int at = 0;
    for (int j = 1; j < 4; ++j)
        if (A[j][j] > A[at][at]) at = j;
    for (int i = 0; i < 4; ++i) q[i] = V[i][at];
}
