/* Sampling of nodal P1 fields at arbitrary points of a mesh, with the exact transpose: the tenth public header of
 * libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, `stream` is a hipStream_t, the return value is DIFFHE_OK or a
 * DIFFHE_E_* status.  diffhe_hip.h, the other eight headers and DIFFHE_ABI_VERSION are unchanged by them; the Python
 * binding keeps them in a table of their own (diffhe/_hip.py, SAMPLE_SIGNATURES).
 *
 * A P1 mesh of dim = 1, 2 or 3 has nodes X (n, dim) and elements el (m, dim + 1).  For a point x and an element e with
 * vertices x_0 .. x_dim the barycentric coordinates are lambda_k(x), k = 0 .. dim: lambda_k for k >= 1 is the ratio of
 * two determinants of the edge vectors x_k - x_0 and x - x_0, evaluated in one fixed fma order, and
 * lambda_0 = (1 - lambda_1) - ... - lambda_dim.  The location rule is
 *
 *   e(x) = the candidate with the LARGEST min_k lambda_k(x), ties to the lowest element id;
 *   x is inside if that minimum is >= -tol; outside points get e = -1, weights 0 and a zero gradient table.
 *
 * The candidates are the elements of the 3^dim cells around the cell of x in a uniform grid (the caller's,
 * diffhe/sampling.py) of ncx * ncy * ncz cells with an edge >= the longest element edge of the mesh: order (m) the element
 * ids sorted by the cell (iz * ncy + iy) * ncx + ix of their centroid, cell_start (ncx * ncy * ncz + 1) the first position
 * of every cell in `order`; pcell (P) the cell of every point, clamped into the grid, porder (P) the point ids sorted by
 * it.  The rule does not depend on the order in which candidates are visited, so every result is a function of the mesh,
 * the points and tol alone, bit for bit.  No atomics anywhere. */
#ifndef DIFFHE_SAMPLE_H
#define DIFFHE_SAMPLE_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For every point p of pts (P, dim): element[p] = e(x_p) or -1; weights (P, dim + 1) the lambda_k of that element as
 * computed (not clamped), in the vertex order of el; gtab (P, dim, dim + 1) the gradients d phi_k / d x_r of that element
 * at [p][r][k]; tested[p] the number of candidates the point was tested against. */
int diffhe_sample_locate(const double* X, const int* el, int dim, int n, int m, const int* order, const int* cell_start,
                         int ncx, int ncy, int ncz, const double* pts, const int* pcell, const int* porder, int P,
                         double tol, int* element, double* weights, double* gtab, int* tested, void* stream);

/* y[p, r, c, b] = sum_k W[p, r, k] u[el[element[p], k], c, b] for r < R, c < C, b < B: W is `weights` with R = 1 (the
 * values) or `gtab` with R = dim (the spatial gradient).  u is read at u[node * u_sn + c * u_sc + b * u_sb], y written at
 * y[p * y_sp + r * y_sr + c * y_sc + b * y_sb]; u and y must not overlap.  Lanes run over samples: coalesced where the
 * sample stride is 1.  An outside point (element -1) reads no u and gets zeros.  Any B: no padding is read or written. */
int diffhe_sample_apply(const int* el, int dim, int n, const int* element, const double* W, int R, int P, const double* u,
                        long long u_sn, long long u_sc, long long u_sb, double* y, long long y_sp, long long y_sr,
                        long long y_sc, long long y_sb, int C, int B, void* stream);

/* The transpose, as a gather: out[i, c, b] = sum over the entries j = p (dim + 1) + k of row i of the incidence list
 * (row_ptr (n + 1), entries ascending within a row: every inside point p whose element has node i as vertex k), and over
 * r < R in ascending order, of W[p, r, k] g[p, r, c, b].  g is read at g[p * g_sp + r * g_sr + c * g_sc + b * g_sb], out
 * written at out[i * o_sn + c * o_sc + b * o_sb]; every entry has one writer.  rows NULL (n_rows 0): every node i < n is
 * visited and every entry of out is written, zeros where the row is empty.  rows (n_rows >= 1 node ids, each once): only
 * those nodes are visited -- the caller has zeroed the rest of out on the same stream; the same bits either way. */
int diffhe_sample_adjoint(const long long* row_ptr, const int* entries, const int* rows, int n_rows, int dim, int n,
                          const double* W, int R, int P, const double* g, long long g_sp, long long g_sr, long long g_sc,
                          long long g_sb, double* out, long long o_sn, long long o_sc, long long o_sb, int C, int B,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_SAMPLE_H */
