/* Block passes of the LOBPCG outer iteration of the eigen, modal and buckling solvers (iteration="lobpcg"): the fifteenth
 * public header of libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, vectors are batch innermost, `stream` is a hipStream_t, the return
 * value is DIFFHE_OK or a DIFFHE_E_* status.  The fourteen other headers and DIFFHE_ABI_VERSION are unchanged by them; the
 * Python binding keeps them in a table of their own (diffhe/_hip.py, LOBPCG_SIGNATURES).
 *
 * Definitions.  The pencil is A x = theta B x per sample, B symmetric positive definite on the free rows, the p <= 16
 * smallest theta wanted.  The basis S = [X | W | P] is ONE (3p, rows, Bp) buffer: column c is the (rows, Bp) vector at
 * c * rows * Bp, X in columns 0 .. p-1, W = T R in p .. 2p-1, P (the previous step) in 2p .. 3p-1; A S and B S are carried
 * as buffers of the same shape.  An entry works on the leading q columns, q one of p, 2p, 3p.  The packed Gram matrices
 * are (nq, Bp), nq = q (q + 1) / 2, entry (i, j), i <= j, at row i q - i (i - 1) / 2 + (j - i).  fp64, no atomics,
 * two-stage reductions in a fixed order and a fixed sweep and pair order in the Ritz step: results are bitwise
 * reproducible. */
#ifndef DIFFHE_LOBPCG_H
#define DIFFHE_LOBPCG_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Row blocks of diffhe_lobpcg_gram (at most 32); 0 for a bad argument. */
int diffhe_lobpcg_gram_blocks(int rows, int Bp);

/* GA[q(i, j)] = s_i . (A s)_j and GB[q(i, j)] = s_i . (B s)_j, i <= j < q <= 48, over the rows with is_bc[row] == 0 (may
 * be NULL).  part: diffhe_lobpcg_gram_blocks(rows, Bp) * 2 * nq * Bp doubles. */
int diffhe_lobpcg_gram(const double* S, const double* AS, const double* BS, const unsigned char* is_bc, int q, int rows,
                       int Bp, double* part, double* GA, double* GB, void* stream);

/* The Ritz step per sample, one wave per sample with its matrices in LDS.  Both matrices are scaled by diag(GB)^-1/2 from
 * either side; GB = L L^T with the relative pivot test 1e-8; cyclic Jacobi (at most `sweeps` sweeps) on L^-1 GA L^-T; the
 * p smallest theta ascending in theta (p, Bp) and C (q, p, Bp), entry (j, c) of sample b at (j p + c) Bp + b, with
 * C^T GA C = diag(theta) and C^T GB C = I.  Where the factorisation fails on the leading m x m block (m = q first) it is
 * tried again on m - p, down to p; used[b] is the m that worked and the rows of C from m on are 0.  used is read too: where
 * 0 < used[b] < q on entry (the last step of the sample fell back) the first m tried is max(used[b], 2p) rounded down to a
 * multiple of p, so a sample that
 * gave up P keeps to [X | W]; the caller sets used to 0 (or 3p) before the first step of a run.  A failure at m = p, or a
 * non-finite entry anywhere in GA or GB, sets flag[b] = 1 and leaves the identity rotation with theta = 0 (flag[b] = 0
 * otherwise). */
int diffhe_lobpcg_ritz(const double* GA, const double* GB, int q, int p, int Bp, int sweeps, double* C, double* theta,
                       int* used, int* flag, void* stream);

/* X' = S C into columns 0 .. p-1 and, where q > p, P' = S C_P (C_P = C with its first p rows zeroed) into columns
 * 2p .. 3p-1 of S2; the same combinations of A S into AS2 and of B S into BS2; R (p, rows, Bp, optional) = A X' - theta
 * B X' from the same registers.  S2, AS2, BS2 are (3p, rows, Bp) and none of them may be an input; their columns p .. 2p-1
 * are not touched.  C as diffhe_lobpcg_ritz leaves it. */
int diffhe_lobpcg_rotate(const double* S, const double* AS, const double* BS, const double* C, const double* theta, int q,
                         int p, int rows, int Bp, double* S2, double* AS2, double* BS2, double* R, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_LOBPCG_H */
