/* Mesh-independent density filter on the elements of any P1 mesh, with its exact adjoint: the ninth public header of
 * libdiffhe_hip.so.
 *
 * The entries below live in the same library and follow the conventions of diffhe_hip.h (which this header includes for
 * the status codes): every array is a device pointer, `stream` is a hipStream_t, the return value is DIFFHE_OK or a
 * DIFFHE_E_* status.  diffhe_hip.h, the other seven headers and DIFFHE_ABI_VERSION are unchanged by them; the Python
 * binding keeps them in a table of their own (diffhe/_hip.py, FILTER_SIGNATURES).
 *
 * For element i with centroid c_i and size v_i (length / area / volume; vol NULL: v = 1) and a radius R > 0
 *
 *   N(i) = { j : |c_i - c_j| < R },    w_ij = R - |c_i - c_j| (weight 0, cone)  or  1 (weight 1, constant),
 *   S_i  = sum_{j in N(i)} w_ij v_j,
 *   forward:  y_i = (sum_{j in N(i)} w_ij v_j x_j) / S_i,        adjoint:  y_j = v_j sum_{i in N(j)} w_ij x_i / S_i.
 *
 * N is symmetric and |c_i - c_j| is computed in one fixed order over the components, so it is bitwise symmetric in
 * (i, j): the adjoint is a gather over the same table with the same weights.  The weights are not stored: the table is the
 * neighbour ids alone (4 B per entry), in ascending order of j within a row, which makes every sum -- S included -- a
 * function of the mesh and R alone.  No atomics anywhere: every result is bitwise reproducible.
 *
 * Binning (the caller's, diffhe/filters.py): a uniform grid of ncx * ncy * ncz cells with an edge >= R; cell_of (m) the
 * cell (iz * ncy + iy) * ncx + ix of every element, order (m) the element ids sorted by cell and, within a cell,
 * ascending; cell_start (ncx * ncy * ncz + 1) the first position of every cell in `order`.  The neighbours of an element
 * are searched in the 3^dim cells around its own.  cent is (dim, m), dim = 1, 2 or 3. */
#ifndef DIFFHE_FILTER_H
#define DIFFHE_FILTER_H

#include "diffhe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* count[i] = |N(i)| (it counts i itself: >= 1). */
int diffhe_filter_count(const double* cent, int dim, int m, const int* cell_of, const int* order, const int* cell_start,
                        int ncx, int ncy, int ncz, double R, int* count, void* stream);

/* With row_ptr (m + 1) the exclusive prefix sum of count: nbr[row_ptr[i] ... row_ptr[i + 1]) = N(i) in ascending order,
 * S[i] summed in that order and inv_S[i] = 1 / S[i]. */
int diffhe_filter_fill(const double* cent, const double* vol, int dim, int m, const int* cell_of, const int* order,
                       const int* cell_start, int ncx, int ncy, int ncz, double R, int weight, const long long* row_ptr,
                       int* nbr, double* S, double* inv_S, void* stream);

/* y = H x (adjoint 0) or H^T x (adjoint 1) for B >= 1 fields: the value of element e and sample b is read at
 * x[e * x_se + b * x_sb] and written at y[e * y_se + b * y_sb]; x and y must not overlap.  Lanes run over samples:
 * coalesced where the sample stride is 1 (from 64 samples on, the neighbour, its centroid, size and weight are computed
 * once per wave); any other strides are correct, not coalesced.  Any B: no padding is read or written. */
int diffhe_filter_apply(const double* cent, const double* vol, int dim, int m, const long long* row_ptr, const int* nbr,
                        const double* inv_S, double R, int weight, int adjoint, const double* x, long long x_se,
                        long long x_sb, double* y, long long y_se, long long y_sb, int B, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFHE_FILTER_H */
