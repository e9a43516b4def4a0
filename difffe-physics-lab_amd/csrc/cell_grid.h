// The uniform cell grid that bins the elements of a mesh (diffhe/cellgrid.py) as the density filter and the point sampler
// walk it: cell c = (z * ncy + y) * ncx + x, and the items of cell c are order[cell_start[c] .. cell_start[c + 1]).
// Index arithmetic only (DIFFHE_HD, as common.h): a host compiler may include this header.
#pragma once
#include <limits.h>

#include "launch.h"

namespace diffhe {

struct Grid {
  int ncx, ncy, ncz;
};

// what the entries refuse: an empty grid, layers in a direction the mesh does not have, a cell index beyond int32
DIFFHE_HD inline bool bad_grid(int dim, int ncx, int ncy, int ncz) {
  return ncx < 1 || ncy < 1 || ncz < 1 || (dim < 2 && ncy != 1) || (dim < 3 && ncz != 1) ||
         (i64)ncx * ncy * ncz >= INT_MAX;
}

struct Cell {
  int x, y, z;
};

DIFFHE_HD inline Cell cell_at(const Grid& g, int c) { return Cell{c % g.ncx, (c / g.ncx) % g.ncy, c / (g.ncx * g.ncy)}; }

// The 3^DIM neighbourhood of cell c, clipped to the grid, row by row in ascending (z, y): f(c0, c1) with the first and
// the last cell of the row.  They are consecutive cell indices, so order[cell_start[c0] .. cell_start[c1 + 1]) is the
// row's items as ONE range.
template <int DIM, class F>
DIFFHE_HD inline void for_each_neighbour_row(const Grid& g, int c, F&& f) {
  const Cell at = cell_at(g, c);
  const int x0 = at.x > 0 ? at.x - 1 : 0, x1 = at.x + 1 < g.ncx ? at.x + 1 : g.ncx - 1;
  for (int dz = (DIM > 2 ? -1 : 0); dz <= (DIM > 2 ? 1 : 0); ++dz) {
    const int z = at.z + dz;
    if (z < 0 || z >= g.ncz) continue;
    for (int dy = (DIM > 1 ? -1 : 0); dy <= (DIM > 1 ? 1 : 0); ++dy) {
      const int y = at.y + dy;
      if (y < 0 || y >= g.ncy) continue;
      const i64 base = ((i64)z * g.ncy + y) * g.ncx;
      f(base + x0, base + x1);
    }
  }
}

// the same cells one by one, in ascending (z, y, x): f(cell)
template <int DIM, class F>
DIFFHE_HD inline void for_each_neighbour_cell(const Grid& g, int c, F&& f) {
  for_each_neighbour_row<DIM>(g, c, [&](i64 c0, i64 c1) {
    for (i64 cc = c0; cc <= c1; ++cc) f(cc);
  });
}

}  // namespace diffhe
