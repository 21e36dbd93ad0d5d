// The sweeps of the cyclic Jacobi solver (jacobi3.h) and the choice of the smallest eigenvalue, included as TEXT where a kernel has its
// covariance, for the reason knn_cells_search.h gives: as a function -- the fifteen doubles by reference, or the matrix by value and the
// seven results returned in a struct -- the same statements compiled to other machine code in both kernels (by reference, equal VGPR
// counts and 80 for 88 bytes of scratch in mls_project_kernel at KMAX 8), and nobody has timed that code.
//
// Reads and overwrites, from the including scope: double a00, a11, a22, a01, a02, a12, the symmetric matrix; afterwards the diagonal
// holds the eigenvalues (unordered) and the off-diagonals what at most 12 sweeps left of them.  Defines:
//   double v00 .. v22   the eigenvectors, v[row][column]            double l0, ex, ey, ez   the smallest eigenvalue (ties: the lowest
//                                                                                           column) and its column, not normalised
// No include guard on purpose: once per kernel.
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        sym3_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0, 1), r = 2
        sym3_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2), r = 1
        sym3_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2), r = 0
        const double scale = fabs(a00) + fabs(a11) + fabs(a22);                 // off-diagonals that no longer change the diagonal
        if (fabs(a01) + scale == scale) a01 = 0.0;
        if (fabs(a02) + scale == scale) a02 = 0.0;
        if (fabs(a12) + scale == scale) a12 = 0.0;
    }
    double l0 = a00, ex = v00, ey = v10, ez = v20;
    if (a11 < l0) { l0 = a11; ex = v01; ey = v11; ez = v21; }
    if (a22 < l0) { l0 = a22; ex = v02; ey = v12; ez = v22; }
