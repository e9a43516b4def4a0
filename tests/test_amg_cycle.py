"""The general path's multigrid cycle, Galerkin products and PCG drivers (csrc/ell_amg.hip, ell_pcg.hip, ell_assemble.hip)
against the numpy model of oracle/amg_model.py.

Every other general-path test solves to convergence, and a converged PCG returns the right u for any symmetric
positive-definite preconditioner: a wrong cycle only costs iterations.  Here the PCG is cut after k = 1 and 3 iterations
(tol = 1e-300, DIFFHE_PCG_NO_FLOOR, max_iter = k): the k-th iterate is a deterministic function of (A, M, b), and
x_1 = alpha M b shows the cycle operator itself.

Tolerances are not picked.  Per case the model runs twice on the CPU, float64 and longdouble with every row sum taken in
reverse order, on the columns SUBSET; the case's tolerance is 16 x the largest difference of the two (relative to |x|_inf
per sample, over k = 1 and 3), never below 2^-46.  The factor covers FMA contraction and the block-partial summation order,
which the model does not reproduce.  In the fp32-stored cycle the same rule applies to the two fp32-store runs.  The GPU
result is held to the float64 model on every real column and to the longdouble model on the subset.

The tests print every figure before they assert (run with -s); the MEASURED table below the imports records one run.
"""
import functools
import types

import numpy as np
import pytest
import torch

from diffhe import FEMesh, _hip, amg
from oracle import amg_model as am

import test_anisotropic as ta
import test_robin as tr
from test_coefficient_hierarchy import _ell_of_mesh

T64 = torch.float64
DEV = "cuda:0"
EPS = float(np.finfo(np.float64).eps)
TOL_FLOOR = 2.0 ** -46
N_COARSE = 3
KS = (1, 3)

# MEASURED on an MI355X, the largest over k (1 and 3; the Jacobi cases 1, 3 and 6), relative to |x|_inf per sample:
# the spread of the two model runs, the tolerance derived from it, the GPU's distance from the float64 model (all
# columns) and from the longdouble model (subset), and the largest |relres - model| over its bound.  Recorded, not
# asserted: every assertion's numbers come from the CPU.
#   case                                           spread       tol    vs f64     vs ld   relres
#   j32sa-shared-B5of8-fp64-g1-s1.3-dense         1.7e-15   2.7e-14   1.9e-15   9.0e-16  5.7e-04
#   j32sa-shared-B5of8-fp32-g1-s1.3-dense         7.6e-08   1.2e-06   3.3e-09   7.6e-08  2.1e-05
#   j32sa-shared-B64of64-fp64-g1-s1.3-dense       1.3e-15   2.2e-14   3.4e-15   1.3e-15  1.3e-03
#   j32sa-shared-B64of64-fp32-g1-s1.3-dense       2.3e-08   3.6e-07   4.3e-08   1.4e-08  3.9e-05
#   j32sa-shared-B128of128-fp64-g1-s1.3-dense     1.6e-15   2.6e-14   3.5e-15   1.2e-15  1.1e-03
#   j32sa-shared-B128of128-fp32-g1-s1.3-dense     4.1e-08   6.6e-07   6.3e-08   4.1e-08  3.0e-05
#   j32sa-shared-B5of8-fp64-g2-s1.3-dense         2.7e-15   4.3e-14   3.1e-15   9.9e-16  9.9e-04
#   j32sa-shared-B5of8-fp32-g2-s1.3-dense         5.0e-08   8.0e-07   2.8e-08   5.0e-08  2.1e-05
#   j32sa-shared-B64of64-fp64-g2-s1.3-dense       2.5e-15   4.0e-14   4.0e-15   1.0e-15  1.5e-03
#   j32sa-shared-B64of64-fp32-g2-s1.3-dense       5.4e-08   8.6e-07   8.7e-08   5.4e-08  6.1e-05
#   j32sa-shared-B128of128-fp64-g2-s1.3-dense     1.8e-15   2.9e-14   3.6e-15   1.3e-15  1.6e-03
#   j32sa-shared-B128of128-fp32-g2-s1.3-dense     8.8e-08   1.4e-06   8.8e-08   8.6e-08  5.6e-05
#   j32sa-shared-B5of8-fp64-g1-s1.3-sweeps        8.1e-16   1.4e-14   1.8e-15   8.1e-16  1.3e-03
#   j32sa-shared-B5of8-fp32-g1-s1.3-sweeps        8.4e-08   1.3e-06   8.4e-08   3.0e-08  5.5e-05
#   j32sa-shared-B64of64-fp64-g1-s1.3-sweeps      3.0e-15   4.8e-14   3.3e-15   8.6e-16  6.2e-04
#   j32sa-shared-B64of64-fp32-g1-s1.3-sweeps      6.1e-08   9.8e-07   6.0e-08   6.1e-08  2.3e-05
#   j32sa-shared-B128of128-fp64-g1-s1.3-sweeps    2.6e-15   4.1e-14   5.0e-15   1.0e-15  8.4e-04
#   j32sa-shared-B128of128-fp32-g1-s1.3-sweeps    1.0e-07   1.6e-06   7.0e-08   1.0e-07  1.6e-05
#   j32sa-sample-B5of8-fp64-g1-s1.3-sweeps        2.8e-15   4.6e-14   3.0e-15   1.1e-15  4.4e-04
#   j32sa-sample-B5of8-fp32-g1-s1.3-sweeps        2.1e-08   3.4e-07   1.9e-08   2.1e-08  2.2e-05
#   j32sa-sample-B64of64-fp64-g1-s1.3-sweeps      2.6e-15   4.2e-14   3.3e-15   1.2e-15  5.3e-04
#   j32sa-sample-B64of64-fp32-g1-s1.3-sweeps      4.7e-08   7.5e-07   2.8e-08   4.7e-08  2.1e-05
#   j32sa-sample-B128of128-fp64-g1-s1.3-sweeps    2.6e-15   4.2e-14   3.2e-15   1.8e-15  5.2e-04
#   j32sa-sample-B128of128-fp32-g1-s1.3-sweeps    3.9e-08   6.3e-07   4.8e-08   3.9e-08  2.2e-05
#   j32sa-shared-B5of8-fp64-g2-s1.0-sweeps        2.1e-15   3.4e-14   2.0e-15   1.6e-15  9.9e-04
#   j32sa-shared-B5of8-fp32-g2-s1.0-sweeps        5.9e-08   9.4e-07   1.9e-15   5.9e-08  3.2e-05
#   j32sa-shared-B64of64-fp64-g2-s1.0-sweeps      2.0e-15   3.2e-14   4.1e-15   1.1e-15  1.9e-03
#   j32sa-shared-B64of64-fp32-g2-s1.0-sweeps      9.0e-08   1.4e-06   3.0e-15   9.0e-08  6.2e-05
#   j32sa-shared-B128of128-fp64-g2-s1.0-sweeps    4.0e-15   6.4e-14   3.9e-15   9.0e-16  1.0e-03
#   j32sa-shared-B128of128-fp32-g2-s1.0-sweeps    9.7e-08   1.5e-06   3.5e-15   9.7e-08  5.2e-05
#   j32sa-sample-B5of8-fp64-g2-s1.0-sweeps        9.5e-16   1.5e-14   1.7e-15   9.9e-16  6.9e-04
#   j32sa-sample-B5of8-fp32-g2-s1.0-sweeps        7.3e-08   1.2e-06   3.5e-15   7.3e-08  2.1e-05
#   j32sa-sample-B64of64-fp64-g2-s1.0-sweeps      2.6e-15   4.2e-14   2.9e-15   7.7e-16  7.7e-04
#   j32sa-sample-B64of64-fp32-g2-s1.0-sweeps      9.6e-08   1.5e-06   3.1e-15   9.6e-08  2.4e-05
#   j32sa-sample-B128of128-fp64-g2-s1.0-sweeps    1.9e-15   3.1e-14   3.7e-15   8.4e-16  1.1e-03
#   j32sa-sample-B128of128-fp32-g2-s1.0-sweeps    7.2e-08   1.1e-06   4.0e-15   7.2e-08  1.6e-05
#   j32pc-shared-B5of8-fp64-g1-s1.8-dense         1.1e-15   1.7e-14   1.3e-15   1.1e-15  1.0e-03
#   j32pc-shared-B5of8-fp32-g1-s1.8-dense         6.2e-08   1.0e-06   2.1e-15   6.2e-08  5.4e-05
#   j32pc-shared-B64of64-fp64-g1-s1.8-dense       1.3e-15   2.1e-14   3.8e-15   1.2e-15  3.2e-03
#   j32pc-shared-B64of64-fp32-g1-s1.8-dense       7.9e-08   1.3e-06   3.0e-15   7.9e-08  3.5e-05
#   j32pc-shared-B128of128-fp64-g1-s1.8-dense     2.0e-15   3.3e-14   4.0e-15   9.1e-16  1.7e-03
#   j32pc-shared-B128of128-fp32-g1-s1.8-dense     8.7e-08   1.4e-06   3.1e-15   8.7e-08  3.5e-05
#   j32pc-sample-B5of8-fp64-g1-s1.8-sweeps        3.0e-15   4.8e-14   3.5e-15   6.3e-16  7.8e-04
#   j32pc-sample-B5of8-fp32-g1-s1.8-sweeps        5.9e-08   9.4e-07   1.8e-15   5.9e-08  5.1e-05
#   j32pc-sample-B64of64-fp64-g1-s1.8-sweeps      2.1e-15   3.3e-14   3.4e-15   9.4e-16  1.1e-03
#   j32pc-sample-B64of64-fp32-g1-s1.8-sweeps      7.4e-08   1.2e-06   3.2e-15   7.4e-08  3.3e-05
#   j32pc-sample-B128of128-fp64-g1-s1.8-sweeps    1.5e-15   2.4e-14   3.6e-15   7.0e-16  2.2e-03
#   j32pc-sample-B128of128-fp32-g1-s1.8-sweeps    6.4e-08   1.0e-06   3.7e-15   6.4e-08  5.1e-05
#   box12sa-shared-B5of8-fp64-g1-s1.3-dense       1.8e-15   2.9e-14   2.0e-15   3.6e-16  8.5e-04
#   box12sa-shared-B5of8-fp32-g1-s1.3-dense       5.3e-08   8.4e-07   5.5e-08   5.2e-08  6.1e-05
#   box12sa-shared-B64of64-fp64-g1-s1.3-dense     2.1e-15   3.4e-14   4.4e-15   4.3e-16  1.9e-03
#   box12sa-shared-B64of64-fp32-g1-s1.3-dense     5.8e-08   9.2e-07   8.1e-08   5.8e-08  9.2e-05
#   box12sa-shared-B128of128-fp64-g1-s1.3-dense   2.9e-15   4.7e-14   3.4e-15   4.3e-16  1.4e-03
#   box12sa-shared-B128of128-fp32-g1-s1.3-dense   8.6e-08   1.4e-06   1.2e-07   4.0e-08  5.3e-05
#   box12sa-sample-B5of8-fp64-g1-s1.3-sweeps      2.2e-15   3.5e-14   2.0e-15   2.7e-16  7.6e-04
#   box12sa-sample-B5of8-fp32-g1-s1.3-sweeps      4.8e-08   7.6e-07   4.8e-08   4.8e-08  2.8e-05
#   box12sa-sample-B64of64-fp64-g1-s1.3-sweeps    2.2e-15   3.6e-14   3.9e-15   4.7e-16  1.2e-03
#   box12sa-sample-B64of64-fp32-g1-s1.3-sweeps    3.8e-08   6.0e-07   4.9e-08   3.8e-08  1.8e-05
#   box12sa-sample-B128of128-fp64-g1-s1.3-sweeps  2.7e-15   4.3e-14   4.2e-15   3.5e-16  1.2e-03
#   box12sa-sample-B128of128-fp32-g1-s1.3-sweeps  5.1e-08   8.2e-07   6.4e-08   5.1e-08  1.8e-05
#   j100sa-shared-B64of64-fp64-g1-s1.0-dense      6.6e-15   1.1e-13   9.7e-15   3.4e-15  7.4e-04
#   j100sa-shared-B64of64-fp32-g1-s1.0-dense      6.8e-08   1.1e-06   1.5e-12   6.8e-08  7.9e-06
#   j100sa-sample-B64of64-fp64-g1-s1.0-sweeps     7.0e-15   1.1e-13   1.0e-14   1.3e-15  5.0e-04
#   j100sa-sample-B64of64-fp32-g1-s1.0-sweeps     7.1e-08   1.1e-06   5.5e-09   7.1e-08  6.9e-06
#   j32sa-sample-B64of64-fp32-g2-s1.0-sweeps-pipe0  7.7e-08   1.2e-06   2.7e-15   7.7e-08  5.4e-05
#   j32pc-shared-B128of128-fp64-g1-s1.8-dense-pipe0  3.2e-15   5.2e-14   3.2e-15   8.9e-16  1.2e-03
#   box12sa-shared-B64of64-fp32-g1-s1.3-dense-pipe0  7.3e-08   1.2e-06   1.1e-07   7.4e-08  4.2e-05
#   j100sa-shared-B64of64-fp64-g1-s1.0-dense-pipe0  6.4e-15   1.0e-13   9.9e-15   3.0e-15  8.8e-04
#   s1-shared-B64of64-fp64-g1-s1.0-dense          1.7e-15   2.6e-14   3.3e-15   3.5e-16  5.3e-04
#   s1-shared-B64of64-fp32-g1-s1.0-dense          1.6e-15   2.5e-14   3.3e-15   2.7e-16  1.5e-03
#   s1-sample-B64of64-fp32-g1-s1.0-sweeps         1.4e-15   2.2e-14   3.7e-15   3.0e-16  5.8e-04
#   s1-shared-B5of8-fp64-g1-s1.0-dense            2.7e-15   4.4e-14   2.6e-15   2.9e-16  2.8e-04
#   s1-sample-B5of8-fp32-g1-s1.0-sweeps           1.1e-15   1.7e-14   1.1e-15   1.8e-16  1.6e-04
#   s2-shared-B64of64-fp64-g1-s1.3-dense          4.5e-15   7.2e-14   4.6e-15   3.8e-16  2.6e-04
#   s2-shared-B64of64-fp32-g1-s1.3-dense          3.8e-15   6.1e-14   3.8e-15   2.8e-16  7.2e-04
#   s2-sample-B64of64-fp32-g1-s1.3-sweeps         1.4e-15   2.2e-14   2.8e-15   3.6e-16  4.5e-04
#   s2-shared-B5of8-fp64-g1-s1.3-dense            1.2e-15   1.9e-14   1.9e-15   2.7e-16  4.3e-04
#   s2-sample-B5of8-fp32-g1-s1.3-sweeps           1.9e-15   3.1e-14   1.9e-15   1.4e-16  2.3e-04
#   s3-shared-B64of64-fp64-g2-s1.0-dense          1.7e-15   2.7e-14   2.9e-15   4.2e-16  1.1e-03
#   s3-shared-B64of64-fp32-g2-s1.0-dense          2.2e-15   3.6e-14   2.8e-15   2.3e-16  9.7e-04
#   s3-sample-B64of64-fp32-g2-s1.0-sweeps         3.3e-15   5.4e-14   3.6e-15   2.3e-16  2.4e-04
#   s3-shared-B5of8-fp64-g2-s1.0-dense            1.6e-15   2.5e-14   1.4e-15   4.0e-16  7.0e-04
#   s3-sample-B5of8-fp32-g2-s1.0-sweeps           1.9e-15   3.1e-14   1.8e-15   3.1e-16  1.7e-04
#   s4-shared-B64of64-fp64-g1-s1.0-dense          1.5e-15   2.5e-14   3.1e-15   5.6e-16  5.0e-04
#   s4-shared-B64of64-fp32-g1-s1.0-dense          1.7e-10   2.7e-09   1.7e-10   2.7e-16  1.2e-05
#   s4-sample-B64of64-fp32-g1-s1.0-sweeps         3.1e-15   5.0e-14   3.8e-15   5.5e-16  9.5e-05
#   s4-shared-B5of8-fp64-g1-s1.0-dense            3.2e-15   5.1e-14   3.2e-15   4.7e-16  4.4e-05
#   s4-sample-B5of8-fp32-g1-s1.0-sweeps           3.2e-15   5.1e-14   3.2e-15   2.6e-16  8.3e-05
#   s5-shared-B64of64-fp64-g1-s1.8-dense          1.5e-15   2.4e-14   3.2e-15   2.5e-16  9.2e-04
#   s5-shared-B64of64-fp32-g1-s1.8-dense          1.9e-08   3.0e-07   3.8e-11   1.9e-08  1.6e-05
#   s5-sample-B64of64-fp32-g1-s1.8-sweeps         1.5e-08   2.5e-07   4.2e-14   1.5e-08  1.2e-05
#   s5-shared-B5of8-fp64-g1-s1.8-dense            1.5e-15   2.4e-14   1.8e-15   3.0e-16  5.4e-04
#   s5-sample-B5of8-fp32-g1-s1.8-sweeps           2.3e-08   3.7e-07   1.4e-15   2.3e-08  7.0e-06
#   s6-shared-B64of64-fp64-g2-s1.0-dense          1.2e-15   1.9e-14   3.1e-15   5.3e-16  6.6e-04
#   s6-shared-B64of64-fp32-g2-s1.0-dense          1.9e-15   3.0e-14   3.1e-15   2.0e-16  1.0e-03
#   s6-sample-B64of64-fp32-g2-s1.0-sweeps         2.2e-15   3.5e-14   2.8e-15   2.2e-16  1.5e-04
#   s6-shared-B5of8-fp64-g2-s1.0-dense            1.4e-15   2.2e-14   1.2e-15   3.1e-16  2.3e-04
#   s6-sample-B5of8-fp32-g2-s1.0-sweeps           1.6e-15   2.6e-14   1.7e-15   4.3e-16  8.7e-05
#   jacobi-n1020-B64of64-shared-ce1               1.5e-15   2.4e-14   3.0e-15   2.5e-16  4.5e-03
#   jacobi-n1020-B64of64-shared-ce4               1.5e-15   2.4e-14   4.4e-16   2.3e-16  1.9e-04
#   jacobi-n1021-B64of64-shared-ce1               1.9e-15   3.0e-14   2.6e-15   3.3e-16  2.9e-03
#   jacobi-n1021-B64of64-shared-ce4               1.9e-15   3.0e-14   4.8e-16   3.3e-16  1.2e-04
#   jacobi-n1025-B64of64-shared-ce1               1.5e-15   2.3e-14   3.0e-15   3.9e-16  4.3e-03
#   jacobi-n1025-B64of64-shared-ce4               1.5e-15   2.3e-14   4.7e-16   3.9e-16  2.1e-04
#   jacobi-n1021-B64of64-sample-ce1               2.0e-15   3.1e-14   3.6e-15   3.1e-16  1.2e-03
#   jacobi-n1021-B64of64-sample-ce4               2.0e-15   3.1e-14   4.2e-16   2.5e-16  5.4e-05
#   jacobi-n8200-B5of8-shared-ce1                 3.8e-15   6.1e-14   3.7e-15   2.5e-16  1.0e-03
#   jacobi-n8200-B5of8-shared-ce4                 3.8e-15   6.1e-14   3.7e-16   2.5e-16  5.2e-05
#   jacobi-n8200-B5of8-sample-ce1                 1.7e-15   2.7e-14   1.5e-15   4.2e-16  6.2e-04
#   jacobi-n8200-B5of8-sample-ce4                 1.7e-15   2.7e-14   4.1e-16   4.2e-16  1.7e-05
# stopping test (tol = 1e-3, floor on): spread, tol, vs f64, vs ld of the final x; the iteration counts met; status words
#   stop-j32sa-B5of8-fp32=0 cap=40                5.7e-16   1.4e-14   1.1e-15   3.5e-16   iters [1, 2, 4] status (4, 0)
#   stop-j32sa-B5of8-fp32=0 cap=3                 5.7e-16   1.4e-14   1.1e-15   3.3e-16   iters [1, 2, 3] status (3, 1)
#   stop-j32sa-B64of64-fp32=0 cap=40              7.3e-16   1.4e-14   1.7e-15   5.5e-16   iters [1, 2, 3, 4] status (4, 0)
#   stop-j32sa-B64of64-fp32=0 cap=3               7.3e-16   1.4e-14   1.7e-15   5.5e-16   iters [1, 2, 3] status (3, 1)
#   stop-j32sa-B64of64-fp32=1 cap=40              1.6e-08   2.5e-07   3.2e-15   1.6e-08   iters [1, 2, 3, 4] status (4, 0)
#   stop-j32sa-B64of64-fp32=1 cap=3               1.6e-08   2.5e-07   3.2e-15   1.6e-08   iters [1, 2, 3] status (3, 1)
#   stop-j32sa-B128of128-fp32=1 cap=40            1.6e-08   2.5e-07   3.7e-15   1.6e-08   iters [1, 2, 3, 4] status (4, 0)
#   stop-j32sa-B128of128-fp32=1 cap=3             1.6e-08   2.5e-07   3.7e-15   1.6e-08   iters [1, 2, 3] status (3, 1)
# Galerkin kernel, largest |difference| / (8 eps (entries summed) sum |terms|) over all levels and samples:
#   j32sa-Bv1 0.12;  j32pc-Bv1 0.04;  box12sa-Bv1 0.12;  j32sa-Bv8 0.15
#   j32pc-Bv8 0.04;  box12sa-Bv8 0.12;  j32sa-Bv64 0.17;  j32pc-Bv64 0.06
#   box12sa-Bv64 0.14;  j32sa-Bv128 0.18;  j32pc-Bv128 0.06;  box12sa-Bv128 0.14


def _subset(B):
    return np.array(sorted({c for c in (0, 1, 31, 32, B - 1, 64, 127) if c < B}), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------------
# real hierarchies, built once per module
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _real(name):
    """dict(cols, unit (W, n), is_bc, levels (host dicts of diffhe.amg), G: kappa (m, B) -> fine values)."""
    import scipy.sparse as sp
    if name.startswith("j32"):
        mesh = ta._jittered(FEMesh.rectangle(32, 32), 0.2, 4)
    elif name == "box12sa":
        mesh = FEMesh.box(12, 12, 12)
    else:
        mesh = ta._jittered(FEMesh.rectangle(100, 100), 0.2, 4)
    cols, unit, is_bc = _ell_of_mesh(mesh)
    if name.endswith("pc"):
        levels = amg.build_hierarchy(cols, is_bc, min_coarse=16)
    else:
        levels = amg.build_hierarchy_sa(cols, unit, is_bc, min_coarse=64 if name == "j100sa" else 16)
    # the fine matrix is linear in kappa: values = G kappa, G (W n, m) from the element matrices
    W, n = cols.shape
    el = mesh.elements.long()
    npe = el.shape[1]
    k0, _ = tr.element_forms(mesh.nodes.to(T64), el)
    r = el[:, :, None].expand(-1, npe, npe).reshape(-1).numpy()
    c = el[:, None, :].expand(-1, npe, npe).reshape(-1).numpy()
    e = np.repeat(np.arange(el.shape[0]), npe * npe)
    A, eidx = amg._ell_to_csr(cols, np.ones((W, n)))
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.indptr)) * n + A.indices
    pos = np.searchsorted(keys, r.astype(np.int64) * n + c)
    assert np.array_equal(keys[pos], r.astype(np.int64) * n + c)
    keep = ~(is_bc[r] | is_bc[c])
    G = sp.csr_matrix((k0.reshape(-1).numpy()[keep], (eidx[pos][keep], e[keep])), shape=(W * n, el.shape[0]))
    return dict(cols=cols, unit=unit, is_bc=is_bc, levels=levels, G=G, m=el.shape[0])


def _fine_values(H, kind, B, Bp, seed):
    """(W, n) unit values, or (W, n, Bp) of a log-normal kappa field (sigma 0.4) per sample; padding samples kappa = 1."""
    if kind == "shared":
        return H["unit"]
    rng = np.random.default_rng(seed)
    kappa = np.ones((H["m"], Bp))
    kappa[:, :B] = np.exp(0.4 * rng.standard_normal((H["m"], B)))
    W, n = H["cols"].shape
    vals = np.asarray(H["G"] @ kappa).reshape(W, n, Bp)
    vals[0, H["is_bc"], :] = 1.0
    return vals


def _rhs(n, B, seed, is_bc=None):
    """Random right-hand sides whose norms spread over four decades (the fp32 cycle's power-of-two scaling)."""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((n, B)) * 10.0 ** rng.uniform(-2, 2, B)
    if is_bc is not None:
        b[is_bc] = 0.0
    return b


def _host_levels(fine_cols, fine_vals, levels, coarse_vals, dense_inv=None, reserved=None):
    """The level dicts of the model from the fine matrix, the hierarchy dicts and the coarse values of every level."""
    out = [dict(cols=fine_cols, vals=fine_vals)]
    for lv, v in zip(levels, coarse_vals):
        out[-1].update(agg=lv["agg"], p_cols=lv.get("p_cols"), p_vals=lv.get("p_vals"))
        out.append(dict(cols=lv["cols"], vals=v))
    for l, res in enumerate(reserved or ()):
        out[l]["reserved"] = res
    out[-1]["dense_inv"] = dense_inv
    return out


def _cpu_coarse(fine_vals, levels):
    """Coarse values of every level from the Galerkin gather lists, on the CPU."""
    out, v = [], fine_vals
    for lv in levels:
        v = am.galerkin(v, lv["ent_ptr"], lv["contrib"], lv.get("weights")).reshape((lv["W"], lv["n"]) + v.shape[2:])
        out.append(v)
    return out


def _cpu_dense_inv(cols, vals):
    n = cols.shape[1]
    D = np.zeros((n, n))
    np.add.at(D, (np.tile(np.arange(n), cols.shape[0]), cols.reshape(-1)), vals.reshape(-1))
    inv = np.linalg.inv(D)
    return 0.5 * (inv + inv.T)


# ------------------------------------------------------------------------------------------------------------------
# synthetic hierarchies: what no small mesh reaches
# ------------------------------------------------------------------------------------------------------------------
def _random_ell(rng, n, W):
    """Random sparse symmetric strictly diagonally dominant ELL matrix, slot 0 the diagonal, padding slots pointing at
    the row itself with value 0; row 0 (at least) has exactly W entries."""
    cap = W - 1
    assert cap <= n - 1
    nb = [set() for _ in range(n)]

    def link(i, j):
        if i != j and j not in nb[i] and len(nb[i]) < cap and len(nb[j]) < cap:
            nb[i].add(j)
            nb[j].add(i)
    if cap:
        for j in rng.permutation(np.arange(1, n))[:cap]:
            link(0, int(j))
        for i in range(n):
            link(i, (i + 1) % n)
        pairs = rng.integers(0, n, size=(n * min(cap, 12), 2))
        for i, j in pairs:
            link(int(i), int(j))
    assert len(nb[0]) == cap
    cols = np.tile(np.arange(n, dtype=np.int32), (W, 1))
    vals = np.zeros((W, n))
    wgt = {}
    for i in range(n):
        order = rng.permutation(np.array(sorted(nb[i]), dtype=np.int64)) if nb[i] else []
        for k, j in enumerate(order, start=1):
            key = (min(i, int(j)), max(i, int(j)))
            if key not in wgt:
                wgt[key] = -rng.uniform(0.2, 1.0)
            cols[k, i], vals[k, i] = j, wgt[key]
    vals[0] = np.abs(vals[1:]).sum(axis=0) * (1.0 + rng.uniform(0.05, 0.3, n)) + 0.1
    return cols, vals


def _random_transfer(rng, nf, nc, pw, sizes):
    """A random prolongation between two levels.  pw == 0: piecewise-constant aggregation (agg and its member lists);
    else rows of P of width pw with -1 holes, 5% of the rows entirely -1, and columns 0 .. len(sizes) - 1 of P^T with
    exactly the given numbers of members.  Returns the dict of transfer arrays of diffhe.amg's levels."""
    perm = rng.permutation(nf)
    n_dir = max(1, nf // 20)
    free = perm[n_dir:]
    agg = np.full(nf, -1, dtype=np.int64)
    if nc == 1:
        sizes = []
    pos = 0
    for I, s in enumerate(sizes):
        agg[free[pos:pos + s]] = I
        pos += s
    rest, others = free[pos:], np.arange(len(sizes), nc)
    assert len(rest) >= len(others) >= 1
    agg[rest[:len(others)]] = others
    agg[rest[len(others):]] = rng.choice(others, len(rest) - len(others))
    if pw == 0:
        ptr, members = amg.members_csr(agg, nc)
        return dict(agg=agg.astype(np.int32), agg_ptr=ptr, agg_members=members)
    p_cols = np.full((pw, nf), -1, dtype=np.int32)
    p_vals = np.zeros((pw, nf))
    for t, i in enumerate(free):
        cnt = pw if t < 8 else int(rng.integers(1, pw + 1))
        pool = others[others != agg[i]]
        extra = rng.choice(pool, min(cnt - 1, len(pool)), replace=False) if cnt > 1 and len(pool) else []
        ent = np.r_[agg[i], extra].astype(np.int64)
        slots = np.sort(rng.choice(pw, len(ent), replace=False))
        p_cols[slots, i] = rng.permutation(ent)
        p_vals[slots, i] = rng.uniform(0.1, 1.0, len(ent)) * rng.choice([1.0, 1.0, 1.0, -0.5], len(ent))
    k, i = np.nonzero(p_cols >= 0)
    I = p_cols[k, i].astype(np.int64)
    order = np.lexsort((k, i, I))
    ptr = np.zeros(nc + 1, dtype=np.int64)
    np.cumsum(np.bincount(I, minlength=nc), out=ptr[1:])
    return dict(agg=agg.astype(np.int32), agg_ptr=ptr.astype(np.int32), agg_members=i[order].astype(np.int32),
                agg_weights=p_vals[k, i][order], p_cols=p_cols, p_vals=p_vals)


SPECIAL = [130, 65, 64, 63, 9, 8, 1]      # members of the first columns of P^T: both sides of the 8- and 64-member chunks
SYNTHETIC = {   # n per level, W per level, p_width per transfer (0: plain aggregation), reserved per level, sizes, gamma, scale
    "s1": dict(n=(1000, 140, 63), W=(9, 65, 19), pw=(8, 9), res=(0, 2001, 2600), sizes=SPECIAL, gamma=1, scale=1.0),
    "s2": dict(n=(1021, 200, 128), W=(8, 108, 64), pw=(12, 1), res=(2000, 2600, 0), sizes=[], gamma=1, scale=1.3),
    "s3": dict(n=(1000, 150, 40, 1), W=(19, 9, 8, 1), pw=(9, 8, 1), res=(0, 0, 2001, 0), sizes=[], gamma=2, scale=1.0),
    "s4": dict(n=(1021, 129), W=(64, 65), pw=(8,), res=(2600, 0), sizes=SPECIAL, gamma=1, scale=1.0),
    "s5": dict(n=(1000, 64), W=(8, 9), pw=(0,), res=(0, 0), sizes=SPECIAL, gamma=1, scale=1.8),
    "s6": dict(n=(1021, 65), W=(9, 8), pw=(12,), res=(0, 2001), sizes=[], gamma=2, scale=1.0),
}


@functools.lru_cache(maxsize=None)
def _synthetic(name):
    """-> (matrices [(cols, vals)] per level, transfers per level but the last, per-sample scalings (n_l, 128))."""
    spec = SYNTHETIC[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    mats = [_random_ell(rng, n, W) for n, W in zip(spec["n"], spec["W"])]
    # a Galerkin operator grows with the aggregates: without the factor the coarse corrections of these unrelated
    # matrices overshoot, the cycle's norm explodes and so does the rounding spread the tolerance is derived from
    mats = [(c, v * 64.0 ** l) for l, (c, v) in enumerate(mats)]
    trs = [_random_transfer(rng, spec["n"][l], spec["n"][l + 1], pw, spec["sizes"] if l == 0 else [])
           for l, pw in enumerate(spec["pw"])]
    scal = [np.exp(0.2 * rng.standard_normal((n, 128))) for n in spec["n"]]
    return mats, trs, scal


def _synthetic_levels(name, kind, Bp):
    """Model level dicts of a synthetic hierarchy (+ its transfer dicts): per-sample values are D_b A D_b, which keeps
    every level symmetric positive definite and the spectrum of D^-1 A."""
    mats, trs, scal = _synthetic(name)
    spec = SYNTHETIC[name]
    out = []
    for l, (cols, vals) in enumerate(mats):
        v = vals
        if kind == "sample":
            s = scal[l][:, :Bp]
            v = vals[:, :, None] * s[None, :, :] * s[cols]
        lv = dict(cols=cols, vals=v, reserved=spec["res"][l])
        if l < len(trs):
            lv.update(agg=trs[l]["agg"], p_cols=trs[l].get("p_cols"), p_vals=trs[l].get("p_vals"))
        out.append(lv)
    out[-1]["dense_inv"] = _cpu_dense_inv(*mats[-1])     # given whatever n is: n = 129 must fall back to sweeps
    return out, trs


# ------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------
class Case(types.SimpleNamespace):
    @property
    def id(self):
        return "-".join([self.hier, self.kind, f"B{self.B}of{self.Bp}", "fp32" if self.fp32 else "fp64", f"g{self.gamma}",
                         f"s{self.scale}", "dense" if self.dense else "sweeps"] + ([] if self.pipe else ["pipe0"]))

    @property
    def flags(self):
        return _hip.PCG_NO_FLOOR | (_hip.PCG_FP32 if self.fp32 else 0)


def _cases():
    out = []
    batches = ((8, 5), (64, 64), (128, 128))
    # coarse corrections scaled as the solver scales them: 1.3 on smoothed hierarchies, 1.8 with a V-cycle on plain ones
    real = [("j32sa", 1, 1.3, True), ("j32sa", 2, 1.3, True), ("j32sa", 1, 1.3, False), ("j32sa", 2, 1.0, False),
            ("j32pc", 1, 1.8, True), ("box12sa", 1, 1.3, True)]
    for hier, gamma, scale, dense in real:
        for kind in ("shared", "sample"):
            if kind == "sample" and dense and hier == "j32sa":
                continue      # the dense level needs a batch-shared hierarchy: per-sample values run the sweeps once
            for Bp, B in batches:
                for fp32 in (0, 1):
                    out.append(Case(hier=hier, kind=kind, Bp=Bp, B=B, fp32=fp32, gamma=gamma, scale=scale,
                                    dense=dense and kind == "shared", pipe=1, synthetic=False))
    for kind in ("shared", "sample"):
        for fp32 in (0, 1):
            out.append(Case(hier="j100sa", kind=kind, Bp=64, B=64, fp32=fp32, gamma=1, scale=1.0, dense=kind == "shared",
                            pipe=1, synthetic=False))
    # the plain kernels (DIFFHE_ELL_PIPE=0) on one batch of whole waves per mesh
    out += [Case(hier="j32sa", kind="sample", Bp=64, B=64, fp32=1, gamma=2, scale=1.0, dense=False, pipe=0, synthetic=False),
            Case(hier="j32pc", kind="shared", Bp=128, B=128, fp32=0, gamma=1, scale=1.8, dense=True, pipe=0, synthetic=False),
            Case(hier="box12sa", kind="shared", Bp=64, B=64, fp32=1, gamma=1, scale=1.3, dense=True, pipe=0, synthetic=False),
            Case(hier="j100sa", kind="shared", Bp=64, B=64, fp32=0, gamma=1, scale=1.0, dense=True, pipe=0, synthetic=False)]
    for name, spec in SYNTHETIC.items():
        for kind, Bp, B, fp32 in (("shared", 64, 64, 0), ("shared", 64, 64, 1), ("sample", 64, 64, 1), ("shared", 8, 5, 0),
                                  ("sample", 8, 5, 1)):
            out.append(Case(hier=name, kind=kind, Bp=Bp, B=B, fp32=fp32, gamma=spec["gamma"], scale=spec["scale"],
                            dense=kind == "shared", pipe=1, synthetic=True))
    return out


CASES = _cases()
_IDS = [c.id for c in CASES]
assert len(set(_IDS)) == len(_IDS)


# The longdouble run covers a subset of the columns, the float64 model every column.  In the fp32-stored cycle a value that
# lands next to an fp32 rounding boundary is stored one ulp apart by two evaluations of the same mathematics; on the
# smoothed mesh hierarchies this happens in every column (exact ties: 1 * e + x of two floats) and the subset's spread
# shows it, on the synthetic ones it is a rare event of single columns, which the subset then misses while the float64
# model of another column carries it.  Such right-hand sides are replaced: the seed of these cases is moved until the
# float64 and the longdouble model agree on EVERY column to a quarter of the tolerance -- a property of the two
# references alone, checked on the CPU by test_float64_model_holds_on_every_column.
RHS_SALT = {"s3-shared-B64of64-fp32-g2-s1.0-dense": 1, "s3-sample-B64of64-fp32-g2-s1.0-sweeps": 1,
            "s6-sample-B64of64-fp32-g2-s1.0-sweeps": 3}


def _seed(case):
    return sum(map(ord, case.id)) % 100000 + RHS_SALT.get(case.id, 0)


def _cpu_levels(case):
    """Model level dicts of a case with every value computed on the CPU (the mutation check; the GPU tests hand the model
    the coarse values and the dense inverse the device computed)."""
    if case.synthetic:
        levels, _ = _synthetic_levels(case.hier, case.kind, case.Bp)
        return [dict(lv, vals=lv["vals"] if lv["vals"].ndim == 2 else lv["vals"][:, :, :case.B]) for lv in levels]
    H = _real(case.hier)
    fine = _fine_values(H, case.kind, case.B, case.Bp, _seed(case))
    if fine.ndim == 3:
        fine = fine[:, :, :case.B]
    coarse = _cpu_coarse(fine, H["levels"])
    dinv = _cpu_dense_inv(H["levels"][-1]["cols"], coarse[-1]) if case.dense else None
    return _host_levels(H["cols"], fine, H["levels"], coarse, dinv)


def _case_rhs(case):
    n = SYNTHETIC[case.hier]["n"][0] if case.synthetic else _real(case.hier)["cols"].shape[1]
    return _rhs(n, case.B, _seed(case) + 1, None if case.synthetic else _real(case.hier)["is_bc"])


def _run_model(levels, case, b, dtype, reverse, columns, mutate=()):
    m = am.AmgModel(levels, N_COARSE, case.gamma, case.scale, case.flags, dtype=dtype, reverse=reverse, columns=columns,
                    mutate=mutate)
    return m, m.pcg(b, max(KS), keep=KS)


def _rel(x, ref):
    """max_i |x - ref| / |ref|_inf per column."""
    ref = np.asarray(ref, dtype=np.longdouble)
    return np.asarray(np.max(np.abs(np.asarray(x, dtype=np.longdouble) - ref), axis=0) / np.max(np.abs(ref), axis=0),
                      dtype=np.float64)


def _tolerance(r64, rld, ks=KS):
    """16 x the largest difference of the float64 and the longdouble run (x relative to |x|_inf per sample), never below
    2^-46: -> (spread, tol)."""
    sx = max(float(_rel(r64.snap[k][0], rld.snap[k][0]).max()) for k in ks)
    return sx, max(16.0 * sx, TOL_FLOOR)


def _relres_scale(cols, vals, b):
    """What an error of x does to the relative residual, per sample: |relres(x + dx) - relres(x)| <= |A dx|_2 / |b|_2 <=
    sqrt(n) |A|_inf |dx|_inf / |b|_2.  The residual's own evaluation in fp64 adds at most (W + 2) eps |A| |x| per row, the
    same expression with (W + 2) eps in the place of the relative error of x.  -> (factor per sample, that addend)."""
    v = np.abs(vals).sum(axis=0).max(axis=0)
    W, n = cols.shape
    return np.sqrt(n) * v / np.linalg.norm(b, axis=0), (W + 2) * EPS


# ------------------------------------------------------------------------------------------------------------------
# CPU: the model is a multigrid, and the cases tell single defects apart
# ------------------------------------------------------------------------------------------------------------------
def test_hierarchy_shapes_are_the_ones_the_cases_are_about():
    def shape(name):
        H = _real(name)
        return [H["cols"].shape[::-1]] + [(lv["n"], lv["W"]) for lv in H["levels"]]
    assert shape("j32sa") == [(1089, 7), (99, 13), (7, 7)] and _real("j32sa")["levels"][0]["p_cols"].shape[0] == 5
    assert shape("j32pc") == [(1089, 7), (99, 9), (13, 7)]
    box = _real("box12sa")
    assert shape("box12sa")[:2] == [(2197, 15), (67, 36)] and shape("box12sa")[2][0] == 3
    assert box["levels"][0]["p_cols"].shape[0] == 8 and int(np.diff(box["levels"][0]["agg_ptr"]).max()) == 123
    j100 = shape("j100sa")
    assert j100[0] == (10201, 7) and j100[-1][0] == 60


def test_model_is_a_multigrid():
    """pcg run to 1e-10 meets a sparse direct solve, and the cycle's matrix on the 99-node level is symmetric."""
    import scipy.sparse.linalg as spla
    H = _real("j32sa")
    levels = _host_levels(H["cols"], H["unit"], H["levels"], _cpu_coarse(H["unit"], H["levels"]))
    b = _rhs(H["cols"].shape[1], 4, 5, H["is_bc"])
    A, _ = amg._ell_to_csr(H["cols"], H["unit"])
    exact = spla.splu(A.tocsc()).solve(b)
    for gamma, flags in ((1, am.PCG_NO_FLOOR), (2, am.PCG_NO_FLOOR), (1, 0), (1, am.PCG_NO_FLOOR | am.PCG_FP32)):
        model = am.AmgModel(levels, N_COARSE, gamma, 1.0, flags)
        res = model.pcg(b, 60, tol=1e-10)
        assert res.not_converged == 0 and res.its < 25 and float(res.relres.max()) <= 1.5e-10, (gamma, flags, res.its)
        assert float(_rel(res.x, exact).max()) < 1e-8
        if not flags & am.PCG_FP32:
            M = model.cycle_matrix(1)
            assert M.shape == (99, 99) and np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
            assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
    # the Jacobi-preconditioned variant
    res = am.jacobi_pcg(H["cols"], H["unit"], b, 500, tol=1e-10)
    assert res.not_converged == 0 and float(_rel(res.x, exact).max()) < 1e-8


def test_model_galerkin_lists_are_pt_a_p():
    """The gather lists of diffhe.amg restated in numpy give P^T A P (scipy) -- what the CPU side of these tests uses."""
    H = _real("j32sa")
    vals = _fine_values(H, "sample", 3, 4, 11)
    coarse = _cpu_coarse(vals, H["levels"])
    for b in range(4):
        Af = amg._ell_to_csr(H["cols"], np.ascontiguousarray(vals[:, :, b]))[0]
        for lv, vc in zip(H["levels"], coarse):
            ref, bound, _ = _pt_a_p_ell(Af, lv)
            assert np.all(np.abs(vc[:, :, b] - ref) <= bound)
            Af = amg._ell_to_csr(lv["cols"], np.ascontiguousarray(vc[:, :, b]))[0]


def _pt_a_p_ell(Af, lv):
    """(P^T A P scattered into the level's ELL pattern, the per-entry bound 8 eps (entries summed) sum |terms|, the mask of
    the pattern's real entries) by scipy, P from p_cols / p_vals or agg."""
    import scipy.sparse as sp
    nf, nc = Af.shape[0], lv["n"]
    if lv.get("p_cols") is not None:
        k, i = np.nonzero(lv["p_cols"] >= 0)
        P = sp.csr_matrix((lv["p_vals"][k, i], (i, lv["p_cols"][k, i])), shape=(nf, nc))
    else:
        i = np.nonzero(lv["agg"] >= 0)[0]
        P = sp.csr_matrix((np.ones(len(i)), (i, lv["agg"][i])), shape=(nf, nc))
    C = (P.T @ Af @ P).toarray()
    Pa, P1 = abs(P), (P != 0).astype(np.float64)
    S = (Pa.T @ abs(Af) @ Pa).toarray()
    A1 = Af.copy()
    A1.data[:] = 1.0
    cnt = (P1.T @ A1 @ P1).toarray()
    cols = lv["cols"]
    I = np.arange(nc)[None, :]
    real = (np.arange(cols.shape[0])[:, None] == 0) | (cols != I)
    ref = np.where(real, C[np.broadcast_to(I, cols.shape), cols], 0.0)
    rows = np.broadcast_to(I, cols.shape)
    bound = np.where(real, 8.0 * EPS * cnt[rows, cols] * S[rows, cols], 0.0)
    # nothing of P^T A P lies outside the pattern
    mask = np.zeros((nc, nc), dtype=bool)
    mask[rows[real], cols[real]] = True
    assert not np.any(C[~mask])
    return ref, bound, real


def _reference(idx):
    """Per case, on the CPU-computed hierarchy: the float64 and the longdouble run on the subset, and the tolerance."""
    case = CASES[idx]
    levels, b, sub = _cpu_levels(case), _case_rhs(case), _subset(case.B)
    _, r64 = _run_model(levels, case, b, np.float64, False, sub)
    _, rld = _run_model(levels, case, b, np.longdouble, True, sub)
    return levels, b, sub, r64, _tolerance(r64, rld)


# "post_not_reversed" is no defect at all: both post-sweeps are polynomials in D^-1 A applied to the same right-hand side,
#   x'' = (I - w_b D^-1 A)(I - w_a D^-1 A) x + (w_a + w_b - w_a w_b D^-1 A) D^-1 rhs,
# which is symmetric in (w_a, w_b) -- the two orders give the same vector and the same (symmetric) cycle in exact
# arithmetic.  No data can tell that mutant apart; test_post_sweep_order_is_immaterial states it instead.
EQUIVALENT = ("post_not_reversed",)


def _skip_reason(mut, case, probe):
    """Why a mutation is not asked of a case (None: it is)."""
    if mut in EQUIVALENT:
        return "mathematically the same cycle"
    if not probe.applies(mut):
        return "the hierarchy has nothing the mutation would break"
    if mut == "galerkin_value_1e-6" and case.fp32:
        # 1e-6 of one value is 17 ulps of the fp32 store, and the fp32 tolerance is 16 x (the rounding ties of the
        # store, ~2^-24): 100 x that is 1e-4, more than a relative change of 1e-6 of anything can move x
        return "below the resolution of the fp32 store"
    return None


@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_cases_tell_single_defects_apart(idx):
    """Each mutation of the model that applies to the case moves x_1 or x_3 by more than 100 x the case's tolerance."""
    case = CASES[idx]
    levels, b, sub, r64, (spread, tol) = _reference(idx)
    probe = am.AmgModel(levels, N_COARSE, case.gamma, case.scale, case.flags, columns=sub)
    for mut in am.MUTATIONS:
        if _skip_reason(mut, case, probe):
            continue
        _, rm = _run_model(levels, case, b, np.float64, False, sub, mutate=(mut,))
        moved = max(float(_rel(rm.snap[k][0], r64.snap[k][0]).max()) for k in KS)
        assert moved > 100.0 * tol, (case.id, mut, moved, tol, spread)


@pytest.mark.parametrize("idx", [i for i, c in enumerate(CASES) if c.Bp == 8 and not c.fp32], ids=lambda i: _IDS[i])
def test_post_sweep_order_is_immaterial(idx):
    """The order of the two post-sweeps changes nothing but roundings (see EQUIVALENT): the fp64 iterates of the model
    with the weights NOT reversed lie within the case's own tolerance of the model's."""
    case = CASES[idx]
    levels, b, sub, r64, (spread, tol) = _reference(idx)
    _, rm = _run_model(levels, case, b, np.float64, False, sub, mutate=("post_not_reversed",))
    assert max(float(_rel(rm.snap[k][0], r64.snap[k][0]).max()) for k in KS) <= tol


_TIE_FREE = [i for i, c in enumerate(CASES) if c.synthetic and c.fp32 and c.Bp >= 64]


@pytest.mark.parametrize("idx", _TIE_FREE, ids=lambda i: _IDS[i])
def test_float64_model_holds_on_every_column(idx):
    """See RHS_SALT: on the synthetic hierarchies' fp32-stored cases the float64 model of every column lies within a
    quarter of the case's tolerance of the longdouble model of that column."""
    case = CASES[idx]
    levels, b, sub, r64s, (spread, tol) = _reference(idx)
    _, r64 = _run_model(levels, case, b, np.float64, False, None)
    _, rld = _run_model(levels, case, b, np.longdouble, True, None)
    assert max(float(_rel(r64.snap[k][0], rld.snap[k][0]).max()) for k in KS) <= 0.25 * tol
    assert set(RHS_SALT) <= set(_IDS)


def test_every_mutation_applies_to_some_case():
    asked = set()
    for c in {(c.hier, c.gamma, c.scale, c.dense, c.kind, c.fp32): c for c in CASES}.values():
        probe = am.AmgModel(_cpu_levels(c), N_COARSE, c.gamma, c.scale, c.flags, columns=_subset(c.B))
        asked |= {mut for mut in am.MUTATIONS if _skip_reason(mut, c, probe) is None}
    assert asked == set(am.MUTATIONS) - set(EQUIVALENT)


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _upload_level(lv):
    keys = ("cols", "ent_ptr", "contrib", "weights", "agg", "agg_ptr", "agg_members", "agg_weights", "p_cols", "p_vals")
    d = dict(n=lv["n"], W=lv["W"])
    d.update({k: _dev(lv[k]) for k in keys if lv.get(k) is not None})
    return d


@functools.lru_cache(maxsize=None)
def _real_dev(name):
    H = _real(name)
    return _dev(H["cols"]), [_upload_level(lv) for lv in H["levels"]]


def _engine(n, W, cols_dev):
    """diffhe's own set-up code (_Engine.amg_setup) on a stand-in plan: the four attributes it reads."""
    from diffhe.solver import _Engine
    eng = _Engine.__new__(_Engine)
    eng.p = types.SimpleNamespace(n=n, W=W, cols=cols_dev, device=torch.device(DEV), amg_levels=None)
    eng.L = _hip.lib()
    return eng


def _setup_real(case):
    """-> (level array, what keeps it alive, model level dicts read back from the device, Bv)."""
    H = _real(case.hier)
    cols_dev, levels_dev = _real_dev(case.hier)
    fine = _fine_values(H, case.kind, case.B, case.Bp, _seed(case))
    Bv = 1 if fine.ndim == 2 else case.Bp
    W, n = H["cols"].shape
    vals_dev = _dev(fine.reshape(W, n, Bv))
    arr, chain = _engine(n, W, cols_dev).amg_setup(vals_dev, Bv, fp32=bool(case.fp32), levels=levels_dev,
                                                   dense_coarse=case.dense)
    torch.cuda.synchronize()
    assert (chain[-1].get("dense_inv") is not None) == bool(case.dense)
    if case.fp32 and Bv != 1:
        assert all(arr[l].vals32 for l in range(len(chain)))
    coarse = [lv["vals"].cpu().numpy() for lv in chain[1:]]
    coarse = [v[:, :, 0] if Bv == 1 else v[:, :, :case.B] for v in coarse]
    dinv = chain[-1]["dense_inv"].cpu().numpy() if case.dense else None
    host = _host_levels(H["cols"], fine if Bv == 1 else fine[:, :, :case.B], H["levels"], coarse, dinv)
    return arr, (chain, vals_dev), host, Bv


def _check_tables(levels, trs):
    """Every index the kernels will follow lies inside its array (a table built wrong must fail here, not on the device)."""
    for l, lv in enumerate(levels):
        n = lv["cols"].shape[1]
        assert lv["cols"].min() >= 0 and lv["cols"].max() < n and np.array_equal(lv["cols"][0], np.arange(n))
        if l < len(trs):
            t, nc = trs[l], levels[l + 1]["cols"].shape[1]
            assert len(t["agg"]) == n and t["agg"].min() >= -1 and t["agg"].max() < nc
            ptr = t["agg_ptr"]
            assert len(ptr) == nc + 1 and ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == len(t["agg_members"])
            assert t["agg_members"].min() >= 0 and t["agg_members"].max() < n
            if "p_cols" in t:
                assert t["p_cols"].shape == t["p_vals"].shape and t["p_cols"].shape[1] == n
                assert t["p_cols"].min() >= -1 and t["p_cols"].max() < nc and len(t["agg_weights"]) == ptr[-1]


def _setup_synthetic(case):
    levels, trs = _synthetic_levels(case.hier, case.kind, case.Bp)
    _check_tables(levels, trs)
    Bv = 1 if case.kind == "shared" else case.Bp
    arr = (_hip.AmgLevel * len(levels))()
    keep = []
    for l, lv in enumerate(levels):
        W, n = lv["cols"].shape
        t = dict(cols=_dev(lv["cols"].astype(np.int32)), vals=_dev(lv["vals"].reshape(W, n, Bv)))
        arr[l].n, arr[l].W, arr[l].reserved = n, W, int(lv["reserved"])
        arr[l].cols, arr[l].vals = t["cols"].data_ptr(), t["vals"].data_ptr()
        if case.fp32 and Bv != 1:
            t["vals32"] = t["vals"].to(torch.float32)
            arr[l].vals32 = t["vals32"].data_ptr()
        if l < len(trs):
            for key in ("agg", "agg_ptr", "agg_members", "agg_weights", "p_cols", "p_vals"):
                if trs[l].get(key) is not None:
                    t[key] = _dev(trs[l][key])
                    setattr(arr[l], key, t[key].data_ptr())
            if "p_cols" in trs[l]:
                arr[l].p_width = int(trs[l]["p_cols"].shape[0])
        if l == len(levels) - 1:
            t["dense_inv"] = _dev(lv["dense_inv"])
            arr[l].dense_inv = t["dense_inv"].data_ptr()
        keep.append(t)
    host = [dict(lv, vals=lv["vals"] if lv["vals"].ndim == 2 else lv["vals"][:, :, :case.B]) for lv in levels]
    return arr, keep, host, Bv


def _amg_solve(arr, nl, Bv, b_dev, Bp, k, case_or_opts, tol=1e-300, flags=None):
    """diffhe_ell_amg_pcg_solve on outputs pre-filled with garbage -> (x, iters, relres, status[0:2])."""
    from diffhe.plan import _stream, status_buffer
    L = _hip.lib()
    o = case_or_opts
    n = arr[0].n
    work = torch.empty(L.diffhe_ell_amg_workspace_doubles(arr, nl, Bp), dtype=T64, device=DEV)
    x = torch.full((n, Bp), float("nan"), dtype=T64, device=DEV)
    relres = torch.full((Bp,), float("nan"), dtype=T64, device=DEV)
    iters = torch.full((Bp,), -7, dtype=torch.int32, device=DEV)
    st = status_buffer()
    st.fill_(-1)
    L.diffhe_ell_amg_pcg_solve(arr, nl, Bv, b_dev, x, Bp, tol, k, N_COARSE, o.gamma, o.scale,
                               o.flags if flags is None else flags, work, relres, iters, st, _stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), relres.cpu().numpy(), (int(st[0]), int(st[1]))


def _padded(b, Bp):
    out = np.zeros((b.shape[0], Bp))
    out[:, :b.shape[1]] = b
    return out


def _check_against(tag, got, r64, rld, sub, B, tols, k, rscale):
    """One GPU result against the float64 model on every real column and the longdouble model on the subset; padding
    columns exactly 0.  relres: within what the tolerance of x allows (_relres_scale).  Prints the figures before it
    asserts."""
    x, iters, relres, _ = got
    spread, tol = tols
    m64, mld = r64.snap[k], rld.snap[k]
    d64, dld = _rel(x[:, :B], m64[0]), _rel(x[:, sub], mld[0])
    tol_r = (tol + rscale[1]) * rscale[0] * np.max(np.abs(m64[0]), axis=0)
    r64d = np.abs(relres[:B] - m64[2]) / tol_r
    rldd = np.abs(relres[sub] - np.asarray(mld[2], dtype=np.float64)) / tol_r[sub]
    print(f"AMGCYCLE {tag} k={k} spread={spread:.3e} tol={tol:.3e} gpu_vs_f64={d64.max():.3e} gpu_vs_ld={dld.max():.3e} "
          f"relres_vs_f64/bound={r64d.max():.3e} relres_vs_ld/bound={rldd.max():.3e}")
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(relres))
    assert np.array_equal(iters[:B], np.full(B, k)) and np.array_equal(m64[1], np.full(B, k))
    assert not np.any(x[:, B:]) and not np.any(iters[B:]) and not np.any(relres[B:])
    assert d64.max() <= tol and dld.max() <= tol, (tag, k, float(d64.max()), float(dld.max()), tol)
    assert r64d.max() <= 1.0 and rldd.max() <= 1.0, (tag, k, float(r64d.max()), float(rldd.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=_IDS)
def test_truncated_amg_pcg_is_the_models(idx, monkeypatch):
    case = CASES[idx]
    monkeypatch.setenv("DIFFHE_ELL_PIPE", str(case.pipe))
    arr, keep, host, Bv = (_setup_synthetic if case.synthetic else _setup_real)(case)
    b, sub = _case_rhs(case), _subset(case.B)
    _, r64 = _run_model(host, case, b, np.float64, False, None)
    _, r64s = _run_model(host, case, b, np.float64, False, sub)
    _, rld = _run_model(host, case, b, np.longdouble, True, sub)
    tols = _tolerance(r64s, rld)
    rscale = _relres_scale(host[0]["cols"], host[0]["vals"].reshape(host[0]["cols"].shape + (-1,)), b)
    b_dev = _dev(_padded(b, case.Bp))
    for k in KS:
        got = _amg_solve(arr, len(host), Bv, b_dev, case.Bp, k, case)
        assert got[3] == (k, case.B)         # k iterations run, every real sample still active
        _check_against(case.id, got, r64, rld, sub, case.B, tols, k, rscale)
    del keep


# -- the PCG driver ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jacobi_system(n):
    rng = np.random.default_rng(n)
    cols, vals = _random_ell(rng, n, 7)
    return cols, vals, np.exp(0.2 * rng.standard_normal((n, 64)))


def _cg_solve(cols, vals, b_dev, n, W, Bp, Bv, tol, max_iter, check_every):
    from diffhe.plan import _stream, status_buffer
    L = _hip.lib()
    work = torch.empty(L.diffhe_cg_workspace_doubles(n, Bp), dtype=T64, device=DEV)
    x = torch.full((n, Bp), float("nan"), dtype=T64, device=DEV)
    relres = torch.full((Bp,), float("nan"), dtype=T64, device=DEV)
    iters = torch.full((Bp,), -7, dtype=torch.int32, device=DEV)
    st = status_buffer()
    st.fill_(-1)
    L.diffhe_ell_cg_solve(vals, cols, b_dev, x, n, W, Bp, Bv, tol, max_iter, check_every, work, relres, iters, st,
                          _stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return x.cpu().numpy(), iters.cpu().numpy(), relres.cpu().numpy(), (int(st[0]), int(st[1]))


JACOBI = [(1020, 64, 64, "shared"), (1021, 64, 64, "shared"), (1025, 64, 64, "shared"), (1021, 64, 64, "sample"),
          (8200, 8, 5, "shared"), (8200, 8, 5, "sample")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,Bp,B,kind", JACOBI, ids=[f"n{n}-B{B}of{Bp}-{kind}" for n, Bp, B, kind in JACOBI])
def test_truncated_jacobi_pcg_is_the_models(n, Bp, B, kind):
    """255, 256 and 257 block partials (either side of the switch to cg_slice_kernel) at Bp = 64, n = 8200 at Bp = 8
    (257 partials of 8 nodes per wave); check_every 1 and 4 at max_iter = 6."""
    cols, vals, scal = _jacobi_system(n)
    Bv = 1 if kind == "shared" else Bp
    full = vals if Bv == 1 else vals[:, :, None] * scal[None, :, :Bp] * scal[cols][:, :, :Bp]
    host = full if Bv == 1 else full[:, :, :B]
    b, sub = _rhs(n, B, n + Bp), _subset(B)
    keep = KS + (6,)
    r64 = am.jacobi_pcg(cols, host, b, 6, keep=keep)
    r64s = am.jacobi_pcg(cols, host, b, 6, keep=keep, columns=sub)
    rld = am.jacobi_pcg(cols, host, b, 6, keep=keep, dtype=np.longdouble, reverse=True, columns=sub)
    tols = _tolerance(r64s, rld, keep)
    rscale = _relres_scale(cols, host.reshape(cols.shape + (-1,)), b)
    cols_dev, vals_dev, b_dev = _dev(cols), _dev(full.reshape(7, n, Bv)), _dev(_padded(b, Bp))
    for k, check_every in ((1, 1), (3, 1), (6, 1), (6, 4)):
        got = _cg_solve(cols_dev, vals_dev, b_dev, n, 7, Bp, Bv, 1e-300, k, check_every)
        assert got[3] == (k, B)
        _check_against(f"jacobi-n{n}-B{B}of{Bp}-{kind}-ce{check_every}", got, r64, rld, sub, B, tols, k, rscale)


STOPPING = [("j32sa", 8, 5, 0), ("j32sa", 64, 64, 0), ("j32sa", 64, 64, 1), ("j32sa", 128, 128, 1)]


@functools.lru_cache(maxsize=None)
def _stopping_modes(hier):
    """Eigenvectors V (columns, on the free nodes) of M A for the model's fp64 cycle M of the unit hierarchy: a right-hand
    side A (sum of m of them) makes the PCG converge in exactly m iterations -- the residual stays large for m - 1
    iterations and then drops to rounding level, far across the threshold."""
    H = _real(hier)
    coarse = _cpu_coarse(H["unit"], H["levels"])
    host = _host_levels(H["cols"], H["unit"], H["levels"], coarse, _cpu_dense_inv(H["levels"][-1]["cols"], coarse[-1]))
    M = am.AmgModel(host, N_COARSE, 1, 1.0, am.PCG_NO_FLOOR).cycle_matrix(0)
    A = amg._ell_to_csr(H["cols"], H["unit"])[0].toarray()
    Lc = np.linalg.cholesky(0.5 * (M + M.T))
    lam, Y = np.linalg.eigh(Lc.T @ A @ Lc)
    V = Lc @ Y
    inner = np.abs(V[H["is_bc"]]).max(axis=0) < 1e-10 * np.abs(V).max(axis=0)       # modes that live on the free nodes
    return H, host, A, V[:, inner]


@functools.lru_cache(maxsize=None)
def _stopping_problem(hier, B, fp32):
    """B right-hand sides of 1 .. 5 modes each (the more modes, the rougher), picked on the CPU: of 8 B candidates the
    first B whose r.r / threshold, by the model, stays outside [1/8, 8] at every iteration."""
    H, host, A, V = _stopping_modes(hier)
    rng = np.random.default_rng(17)
    b = np.zeros((A.shape[0], 8 * B))
    for c in range(b.shape[1]):
        pick = rng.choice(V.shape[1], 1 + c % 5, replace=False)
        AV = A @ V[:, pick]
        b[:, c] = (AV / np.linalg.norm(AV, axis=0)).sum(axis=1) * 10.0 ** (c % 3 - 1)
    ratios = np.array(am.AmgModel(host, N_COARSE, 1, 1.0, am.PCG_FP32 if fp32 else 0).pcg(b, 40, tol=1e-3).ratios)
    good = np.nonzero(np.all(np.isnan(ratios) | (ratios < 0.125) | (ratios > 8.0), axis=0))[0]
    assert len(good) >= B, (len(good), B)
    return H, b[:, good[:B]]


@pytest.mark.gpu
@pytest.mark.parametrize("hier,Bp,B,fp32", STOPPING, ids=[f"{h}-B{B}of{Bp}-{'fp32' if f else 'fp64'}" for h, Bp, B, f in STOPPING])
def test_stopping_rule_is_the_models(hier, Bp, B, fp32):
    """tol = 1e-3 with the attainable-accuracy floor on: iters per sample, the status words and the frozen x of the
    stopped samples are the model's, at an iteration cap that stops everything and at one that leaves samples active.
    The data keep r.r / threshold outside [1/4, 4] for every sample at every iteration (asserted here, on the CPU), so a
    rounding difference cannot move a stop."""
    H, b = _stopping_problem(hier, B, fp32)
    case = Case(hier=hier, kind="shared", Bp=Bp, B=B, fp32=fp32, gamma=1, scale=1.0, dense=True, pipe=1, synthetic=False)
    arr, keep, host, Bv = _setup_real(case)
    flags = _hip.PCG_FP32 if fp32 else 0
    sub = _subset(B)
    b_dev = _dev(_padded(b, Bp))
    for cap in (40, 3):
        mk = lambda dtype, rev, cols_: am.AmgModel(host, N_COARSE, 1, 1.0, flags, dtype=dtype, reverse=rev,   # noqa: E731
                                                   columns=cols_).pcg(b, cap, tol=1e-3, keep=(cap,))
        r64, r64s, rld = mk(np.float64, False, None), mk(np.float64, False, sub), mk(np.longdouble, True, sub)
        ratios = np.array(r64.ratios)
        ok = np.isnan(ratios) | (ratios < 0.25) | (ratios > 4.0)
        assert ok.all(), (cap, ratios[~ok])
        assert len(set(r64.iters.tolist())) >= 3, r64.iters          # the samples do stop at different iterations
        assert np.array_equal(r64s.iters, np.asarray(rld.iters)) and np.array_equal(r64.iters[sub], r64s.iters)
        x, iters, relres, status = _amg_solve(arr, len(host), Bv, b_dev, Bp, cap, case, tol=1e-3, flags=flags)
        sx = float(_rel(r64s.x, rld.x).max())
        tol = max(16.0 * sx, TOL_FLOOR)
        d64, dld = _rel(x[:, :B], r64.x), _rel(x[:, sub], rld.x)
        print(f"AMGCYCLE stop-{hier}-B{B}of{Bp}-fp32={fp32} cap={cap} spread={sx:.3e} tol={tol:.3e} "
              f"gpu_vs_f64={d64.max():.3e} gpu_vs_ld={dld.max():.3e} iters={sorted(set(iters[:B].tolist()))} status={status}")
        assert np.array_equal(iters[:B], r64.iters) and not np.any(iters[B:]) and not np.any(x[:, B:])
        assert status == (r64.its, r64.not_converged)
        assert (cap == 3) == (r64.not_converged > 0)
        assert d64.max() <= tol and dld.max() <= tol, (float(d64.max()), float(dld.max()), tol)
    del keep


# -- the Galerkin kernel -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("hier", ["j32sa", "j32pc", "box12sa"])
@pytest.mark.parametrize("Bv", [1, 8, 64, 128])
def test_galerkin_kernel_is_pt_a_p(hier, Bv):
    """diffhe_ell_galerkin on every level (weights given: smoothed aggregation; NULL: plain aggregation) against
    P^T A P by scipy, scattered into the level's ELL pattern, entry by entry, padding slots included (exactly 0)."""
    from diffhe.plan import _stream
    H = _real(hier)
    _, levels_dev = _real_dev(hier)
    L = _hip.lib()
    fine = _fine_values(H, "shared" if Bv == 1 else "sample", Bv, Bv, 100 + Bv)
    W, n = H["cols"].shape
    v_dev = _dev(fine.reshape(W, n, Bv))
    outs = []
    for lv in levels_dev:
        vc = torch.full((lv["W"], lv["n"], Bv), float("nan"), dtype=T64, device=DEV)
        L.diffhe_ell_galerkin(v_dev, lv["ent_ptr"], lv["contrib"], lv.get("weights"), vc, lv["n"], lv["W"], Bv,
                              _stream(torch.device(DEV)))
        outs.append(vc)
        v_dev = vc
    torch.cuda.synchronize()
    assert (hier == "j32pc") == (levels_dev[0].get("weights") is None)
    worst = 0.0
    for b in range(Bv):
        cols_f, vals_f = H["cols"], fine.reshape(W, n, Bv)[:, :, b]
        for lv, vc in zip(H["levels"], outs):
            Af = amg._ell_to_csr(cols_f, np.ascontiguousarray(vals_f))[0]
            got = vc[:, :, b].cpu().numpy()
            ref, bound, real = _pt_a_p_ell(Af, lv)
            assert not np.any(got[~real]), (hier, b)
            assert np.all(np.abs(got - ref) <= bound), (hier, b, float(np.abs(got - ref).max()))
            nz = bound > 0
            worst = max(worst, float(np.max(np.abs(got - ref)[nz] / bound[nz])))
            cols_f, vals_f = lv["cols"], got       # the next level's product is taken of the device's own values
    print(f"AMGCYCLE galerkin-{hier}-Bv{Bv} largest |difference| / bound = {worst:.3e}")
