/*
 * diffhe_hip.h -- C ABI of libdiffhe_hip.so: the MI355X (gfx950) differentiable
 * P1-FEM solve path behind diffhe.DifferentiableFESolver.
 *
 * The reference (danieleschmidt/DiffFE-Physics-Lab) has no FFI of its own: its hot
 * path is three Python methods (diffhe/solver.py:73-98 `_solve_1d`, :104-147
 * `_solve_2d`, :153-183 `_apply_bc_and_solve`) whose adjoint is whatever autograd
 * replays.  Each entry point below replaces a slice of those methods; the slice is
 * cited per function.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - values are fp64, indices int32, sizes `int`/`long long`;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered;
 *   - functions return 0 (DIFFHE_OK) or a negative DIFFHE_E_* code, never throw,
 *     never allocate: workspaces are caller-owned;
 *   - 1D chain path: sample-major (B, n) arrays with an explicit row stride;
 *   - 2D/general path: node-major, batch-innermost arrays `(n, Bp)`:
 *     element (i, b) lives at `i * Bp + b`, Bp = padded batch (power of two <= 64
 *     or a multiple of 64).  The mesh pattern is shared by the whole batch.
 */
#ifndef DIFFHE_HIP_H
#define DIFFHE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DIFFHE_ABI_VERSION 8

#define DIFFHE_OK 0
#define DIFFHE_E_BADARG (-1)
#define DIFFHE_E_LAUNCH (-2)   /* a HIP launch/runtime call failed */
#define DIFFHE_E_TOOBIG (-3)   /* problem exceeds what this entry point supports */
#define DIFFHE_E_BATCHPAD (-4) /* Bp is not a power of two <= 64 or a multiple of 64 */

int diffhe_abi_version(void);
const char* diffhe_status_string(int status);
/* hipGetLastError()-style text of the last DIFFHE_E_LAUNCH on this thread. */
const char* diffhe_last_hip_error(void);

/* Algorithmic-byte accounting of the solve path.  Every kernel launch of the lattice path and of the shared
 * set-up / layout kernels adds the unique bytes it must read + write once (batch-shared
 * data counts 0; per-sample matrices count their stored diagonals) to a process-wide counter.
 * Returns the totals since the last reset; reset != 0 clears them.  bench.py divides the bytes of the timed
 * steps by their duration: the step-level fraction of the HBM roofline. */
int diffhe_traffic_account(int reset, double* bytes_host, long long* launches_host);

/* ------------------------------------------------------------------------------
 * 1D chain path (elements[e] = (e, e+1)).  Fused assemble + solve; K is never
 * materialised.  The P1 stiffness of a chain is a weighted path-graph Laplacian:
 * its inverse is two prefix sums (flux scan, then potential scan), evaluated per
 * Dirichlet-delimited segment by one workgroup per (segment, sample).
 *
 * Replaces solver.py:73-98 (element integrals h_e, k_e = kappa/h_e, lumped load
 * h_e/2 f_i) + solver.py:153-183 (elimination, solve, scatter-back).
 *
 *   x        (n)            node coordinates
 *   kappa    kappa[b*kappa_sb + e*kappa_se]   (strides 0 broadcast)
 *   rhs      rhs[b*rhs_sb + i]  nodal forcing f (rhs_sb = 0 shares one f)
 *   seg      (n_seg, 3) int32: first node, last node, flags
 *            (bit0: first node is Dirichlet, bit1: last node is Dirichlet)
 *   g        (n) Dirichlet values (0 at free nodes)
 *   u        (B, n) out, row stride ldu
 *   max_seg_len  elements of the longest segment (1 .. n-1): selects the kernel.  Segments up to
 *            10 240 elements are solved in registers; longer ones stage through `stage`.
 *   flags    DIFFHE_CHAIN_REFERENCE_ORDER: solve the system the reference ASSEMBLED in fp64 --
 *            weights k_e = fl(kappa_e/h_e), diagonal fl(k_{i-1} + k_i) (solver.py:88-92), load
 *            fl(fl(h/2) f_i) summed in element order (solver.py:95-96) -- by correcting the exact
 *            scan solution to first order in the diagonal's rounding error (a second scan in the
 *            same kernel; see chain1d.hip).  Measured 7e-12 from torch.linalg.solve at N = 1e4,
 *            where the plain scan -- which solves the unrounded weighted Laplacian to 1e-15 -- is
 *            4e-10 away.  0: plain scan.
 *   stage    global staging buffer of diffhe_chain1d_stage_doubles(...) doubles (0 when every
 *            segment fits the register kernel: may be NULL then; DIFFHE_E_TOOBIG if needed and NULL)
 * ---------------------------------------------------------------------------- */
#define DIFFHE_CHAIN_REFERENCE_ORDER 1

long long diffhe_chain1d_stage_doubles(int n, int B, int max_seg_len, int flags);

int diffhe_chain1d_solve(const double* x, const double* kappa, long long kappa_sb, long long kappa_se,
                         const double* rhs, long long rhs_sb, const int* seg, int n_seg, const double* g,
                         double* u, long long ldu, int n, int B, int max_seg_len, int flags, double* stage,
                         void* stream);

/* Adjoint of the above (reverse of solver.py:89-96,169-181):
 *   lambda = K_free^{-1} gbar_free (lambda = 0 on Dirichlet nodes);
 *   df[b,i]      = lambda_i * sum_{e ni i} h_e/2
 *   dkappa_e[b,e] = -(lambda_{e+1}-lambda_e)(u_{e+1}-u_e)/h_e        (optional, may be NULL)
 *   dkappa_part[b*n_seg + s] = sum over the elements of segment s of dkappa_e
 * With DIFFHE_CHAIN_REFERENCE_ORDER lambda is the solution of the reference's rounded matrix (what
 * autograd's LinalgSolveExBackward computes), same correction as the forward solve.
 */
int diffhe_chain1d_adjoint(const double* x, const double* kappa, long long kappa_sb, long long kappa_se,
                           const double* gbar, long long gbar_sb, const double* u, long long ldu,
                           const int* seg, int n_seg, double* df, long long lddf, double* dkappa_e,
                           long long lddk, double* dkappa_part, int n, int B, int max_seg_len, int flags,
                           double* stage, void* stream);

/* ------------------------------------------------------------------------------
 * General P1 path (any 1D/2D mesh, P1 tetrahedra in 3D): per-element integrals, deterministic gather
 * assembly into a batch-shared ELL pattern, Dirichlet elimination, batched PCG.
 * ---------------------------------------------------------------------------- */

/* Element integrals, batch-invariant (solver.py:84-88 1D; solver.py:119-139 2D; dim = 3: P1 tetrahedra, ours).
 *   coords (dim, n) SoA; elems (npe, m) SoA int32, npe = dim + 1
 *   k0 (npe*npe, m): unit-kappa local stiffness, entry p*npe+q (3D: g_p . g_q / (36 V), g_p = 6 V grad phi_p)
 *   m0 (npe*npe, m): local load map (1D: diag h/2; 2D: area/9 everywhere; 3D: V/16 everywhere)
 *   degenerate triangles (area < 1e-15, solver.py:120-121) and tetrahedra (6 V <= 1e-12 l^3, l the longest edge
 *   from the first vertex) get zeros. */
int diffhe_p1_element_integrals(const double* coords, const int* elems, int dim, int n, int m,
                                double* k0, double* m0, void* stream);

/* Deterministic row-gather assembly with fused Dirichlet elimination.
 * Replaces the scatter-add of solver.py:89-92 / :137-140 and the elimination of
 * solver.py:165-171.
 *   local     (npe*npe, m) local matrices (k0 or m0)
 *   kappa     kappa[e*kappa_se + b*kappa_sb] or NULL for kappa == 1
 *   ent_ptr   (n*W + 1) CSR over ELL entries (row i, slot k) -> contributions
 *   contrib   packed (e * 64 + p*npe+q), npe <= 6
 *   cols      (W, n) column id of entry (row i, k) at k*n + i; entry 0 = diagonal;
 *             unused entries point at the row itself
 *   store_slot (W) or NULL: entry k is stored at vals[(store_slot[k], i, b)]; -1 = not
 *             stored (lower triangle of the symmetric-diagonal lattice format: such
 *             entries only feed the Dirichlet lift).  NULL = identity (ELL).
 *   is_bc     (n) bytes or NULL (no elimination: raw K);  g (n) Dirichlet values
 *   vals      out (W, n, Bv); Bv = padded batch, or 1 when kappa is batch-shared
 *   lift      out (n, Bv) or NULL: lift_i = sum_{j in bc} K_ij g_j (0 on Dirichlet rows);
 *             Dirichlet rows become identity rows, couplings to Dirichlet columns 0.
 */
int diffhe_ell_assemble_rows(const double* local, const double* kappa, long long kappa_se, long long kappa_sb,
                             const int* ent_ptr, const int* contrib, const int* cols, const int* store_slot,
                             const unsigned char* is_bc, const double* g, double* vals, double* lift, int n, int m,
                             int W, int Bv, void* stream);

/* diffhe_ell_assemble_rows for FEMesh.rectangle connectivity (reference mesh.py:100-105) without the gather lists: the
 * contributions of the seven entry kinds (0, +1, +W, +nx, -1, -W, -nx; the first `nd` stored as symmetric diagonals
 * (nd, n, Bv), the rest feeding the Dirichlet lift) are written into the kernel in the element order of the
 * reference's loops (solver.py:137-140) -- bitwise the values of diffhe_ell_assemble_rows with the lattice lists, each
 * kappa_e read once per node.  local: (9, m) unit element matrices, or -- local_compact != 0, ABI v7 -- (9, 2): one matrix
 * per triangle orientation (element parity) of a lattice whose triangles are congruent bit for bit (the caller has
 * compared the columns); kappa (optional) strided by kappa_se per element and kappa_sb per sample. */
int diffhe_lattice_assemble_rows(const double* local, int local_compact, const double* kappa, long long kappa_se,
                                 long long kappa_sb, const unsigned char* is_bc, const double* g, double* vals,
                                 double* lift, int nx, int ny, int nd, int Bv, void* stream);
/* The same gather assembly in the REFERENCE'S OPERATION ORDER: tnum (npe*npe, m) holds t = b_p b_q + c_p c_q (2D;
 * +-1 in 1D), den (m) holds 4 area (2D; h in 1D), and every contribution is (kappa * t) / den with each operation
 * rounded on its own (no contracted multiply-adds, a true division), added in element order -- solver.py:88-92,
 * :139-140 verbatim.  The stored values and the lifting terms are then bit-identical to the reference's K; used
 * wherever the matrix is assembled with kappa folded in (everything except the factored per-sample-scalar mode). */
int diffhe_ell_assemble_rows_ref(const double* tnum, const double* den, const double* kappa, long long kappa_se,
                                 long long kappa_sb, const int* ent_ptr, const int* contrib, const int* cols,
                                 const int* store_slot, const unsigned char* is_bc, const double* g, double* vals,
                                 double* lift, int n, int m, int W, int Bv, void* stream);

/* Element-parallel assembly with fp64 global atomics (the literal scatter-add of
 * solver.py:89-92 / :137-140): element integrals are computed from coords and
 * staged in LDS, then scattered for all Bp samples.  `vals` must be zeroed by the
 * caller; `slot_of` (npe*npe, m) gives the ELL slot of entry (p,q) of element e (dim 3: -1 = the entry was
 * pruned from the pattern as a structural zero, skipped).
 * No Dirichlet handling (use diffhe_ell_apply_dirichlet). */
int diffhe_ell_assemble_atomic(const double* coords, const int* elems, int dim, const double* kappa,
                               long long kappa_se, long long kappa_sb, const int* slot_of, double* vals, int n,
                               int m, int W, int Bp, void* stream);

/* Dirichlet elimination on an assembled ELL matrix (solver.py:165-171). */
int diffhe_ell_apply_dirichlet(const int* cols, const unsigned char* is_bc, const double* g, double* vals,
                               double* F, int n, int W, int Bp, void* stream);

/* y = is_bc ? 0 : (M x - sub_scale[b] * sub) for a batch-shared ELL matrix (values (W, n)): the
 * load vector F = M f (solver.py:95-96 / :143-145) minus the Dirichlet lift
 * (solver.py:166-169), and the adjoint df = M^T lambda (M symmetric; sub = is_bc = NULL).
 *   sub (n, sub_B) with sub_B == Bp or 1 (batch-shared), or NULL; sub_scale (Bp) or NULL (= 1) */
int diffhe_ell_spmv_shared(const double* vals, const int* cols, const double* x, const double* sub, int sub_B,
                           const double* sub_scale, const unsigned char* is_bc, double* y, int n, int W, int Bp,
                           void* stream);

/* Batched Jacobi-preconditioned CG on (W, n, Bv) ELL values, all samples at once.
 * Replaces torch.linalg.solve (solver.py:174) and, for the adjoint, the solve in
 * its autograd backward.  x is the output (initial guess 0).
 *   vals     (W, n, Bv), Bv = Bp or 1 (matrix shared by the batch)
 *   work     diffhe_cg_workspace_doubles(n, Bp) doubles
 *   status_host  pinned host int[4]: [0] iterations run, [1] samples not converged, [2] scratch,
 *            [3] scratch inside diffhe_lattice_pcg_solve, which leaves a count there (see it); untouched by the others
 *   relres   (Bp) out: true relative residual |b - A x| / |b| per sample
 *   iters    (Bp) out: iterations each sample was active
 */
long long diffhe_cg_workspace_doubles(int n, int Bp);
int diffhe_ell_cg_solve(const double* vals, const int* cols, const double* b, double* x, int n, int W, int Bp,
                        int Bv, double tol, int max_iter, int check_every, double* work, double* relres,
                        int* iters, int* status_host, void* stream);

/* ------------------------------------------------------------------------------
 * Aggregation multigrid for general meshes.  The hierarchy (aggregates, coarse ELL patterns,
 * Galerkin gather lists) is batch-shared and built on the host once per mesh; coarse VALUES are
 * P^T A P with piecewise-constant P = sums of fine entries, rebuilt per solve / per sample.
 * ---------------------------------------------------------------------------- */
typedef struct diffhe_amg_level {
  int n, W;                /* nodes and ELL width of this level */
  const double* vals;      /* (W, n, Bv) */
  const int* cols;         /* (W, n) */
  const int* agg;          /* (n) node -> node of the NEXT level, -1 = none (Dirichlet); NULL on the last level */
  const int* agg_ptr;      /* (n_next + 1) CSR of the members of each next-level node; NULL on the last level */
  const int* agg_members;  /* node ids, grouped by aggregate */
  const float* vals32;     /* optional fp32 copy of vals, read by the fp32 cycle when Bv == Bp (may be NULL) */
  /* SMOOTHED aggregation (ABI v6; all NULL / 0 = piecewise-constant aggregation as above): the batch-shared
   * prolongation P = (I - omega D_1^-1 A_1) P_0 to the NEXT level, as ELL rows, and its transpose as weights of the
   * CSR above (agg_ptr / agg_members then list the support of each next-level node's column of P) */
  const double* agg_weights; /* (nnz P) weight of each entry of agg_members */
  const int* p_cols;         /* (p_width, n) next-level node of each entry of P's row, -1 = none */
  const double* p_vals;      /* (p_width, n) */
  int p_width;
  /* 0, or 1000 x an upper bound of lambda_max(D^-1 A) of this level (coefficient-aware hierarchy): above 2000 the
   * cycle's Jacobi weights, Chebyshev for [0.5, 2], are scaled by 2000 / reserved on this level */
  int reserved;
  /* LAST level of a batch-shared hierarchy (Bv == 1), optional: the (n, n) row-major INVERSE of this level's matrix,
   * n <= 128 -- the level is then solved by one dense product instead of n_coarse Jacobi sweeps (NULL: sweeps) */
  const double* dense_inv;
} diffhe_amg_level;

/* vals_coarse[(k*n_coarse + I)*Bv + b] = sum of weights[c] * vals_fine[contrib[c]*Bv + b], c in ent_ptr[k*n_coarse+I] ..
 * (weights NULL = 1: piecewise-constant aggregation; smoothed aggregation: weights[c] = P_iI P_jJ, ABI v6) */
int diffhe_ell_galerkin(const double* vals_fine, const int* ent_ptr, const int* contrib, const double* weights,
                        double* vals_coarse, int n_coarse, int W_coarse, int Bv, void* stream);
/* Batched CG preconditioned by one aggregation-multigrid cycle: V(2,2) Chebyshev-weighted Jacobi,
 * `gamma` coarse corrections per level (2 = W-cycle), coarse correction scaled by `scale`, n_coarse
 * sweeps on the last level.  Replaces torch.linalg.solve (solver.py:174) on general meshes.
 * flags: DIFFHE_PCG_FP32: the cycle stores its vectors in fp32 (arithmetic fp64 in registers) and reads levels[].vals32
 * where given; the CG vectors, residuals and dot products stay fp64.  DIFFHE_PCG_NO_FLOOR: stop on `tol` alone.
 * Arguments as diffhe_ell_cg_solve; levels is a HOST array.  The stop is floored like
 * diffhe_lattice_pcg_solve's: sample b stops at |r| <= max(tol |b|, 0.5 u |A_b| |x_b|), with the running
 * iterate x (this path starts from 0). */
long long diffhe_ell_amg_workspace_doubles(const diffhe_amg_level* levels, int n_levels, int Bp);
int diffhe_ell_amg_pcg_solve(const diffhe_amg_level* levels, int n_levels, int Bv, const double* b, double* x, int Bp,
                             double tol, int max_iter, int n_coarse, int gamma, double scale, int flags,
                             double* work,
                             double* relres, int* iters, int* status_host, void* stream);

/* One application of the batched operator, y = A x, with the per-sample dots x.y left as
 * block partials in `part` (diffhe_grad_kappa_blocks(n, Bp) * Bp doubles): the very kernel
 * the CG loop launches once per iteration, exposed so it can be timed and tested alone. */
int diffhe_ell_apply(const double* vals, const int* cols, const double* x, double* y, double* part, int n, int W,
                     int Bp, int Bv, void* stream);

/* ------------------------------------------------------------------------------
 * Lattice fast path: meshes with the connectivity of FEMesh.rectangle (mesh.py:100-105).
 * Operator = symmetric diagonals D0 (i,i), D1 (i,i+1), D2 (i,i+nx+1), D3 (i,i+nx; only when
 * nd == 4), values (nd, n, Bv) produced by diffhe_ell_assemble_rows with
 * store_slot = {0,1,2,3|-1,-1,-1,-1}.  Level l+1 halves level l in x, in y (semi-coarsening of
 * anisotropic meshes) or in both.
 * ---------------------------------------------------------------------------- */
typedef struct diffhe_mg_level {
  int nx, ny;                  /* elements per direction; n = (nx+1)*(ny+1) */
  int nd;                      /* stored diagonals: 3 or 4 */
  int reserved;
  const double* vals;          /* (nd, n, Bv) */
  const unsigned char* is_bc;  /* (n) */
  const float* vals32;         /* optional fp32 copy of vals (NULL = none): read by the fp32-stored
                                  V-cycle (Bv == Bp: per-sample copies; Bv == 1: see rdiag32); the outer CG always
                                  applies the fp64 values */
  const void* dense_inv;       /* LAST level only, Bv == 1, optional: dense inverse (n, n) row-major of this level's
                                  matrix (identity rows -> zero rows), fp32 when the V-cycle is stored fp32 else
                                  fp64.  The coarsest-level solve is then ONE dense product per cycle (scaled by
                                  1 / scale[b]) instead of the Chebyshev iteration; NULL = Chebyshev */
  const double* shift;         /* optional (n), batch-shared: the level operator is scale[b] * K + diag(shift) on the
                                  free rows (reaction term c M_L of a FACTORED operator; must be 0 on Dirichlet rows and
                                  must not be combined with dense_inv); NULL = none */
  const float* rdiag32;        /* optional (n), Bv == 1 only (ABI v6): fp32 reciprocal of the main diagonal vals[0].  Given
                                  together with vals32 (here (nd, n): fp32 copy of the SHARED values) it lets the
                                  fp32-stored V-cycle run its two-samples-per-lane strip kernels (packed fp32
                                  arithmetic, no division); needs mask32, Bp % 128 == 0 and no shift; NULL = the
                                  fp64-in-registers kernels */
  const float* mask32;         /* with rdiag32: (n) 0.0f on Dirichlet rows, 1.0f elsewhere (is_bc as scalar-loadable floats) */
  const void* offdiag16;       /* optional, Bv == Bp only (ABI v6): fp16 off-diagonals (nd - 1, n, Bv), those of sample b
                                  divided by offdiag_scales[b]; vals32 is then the (n, Bv) fp32 main diagonal adjusted to
                                  keep every row sum of `vals` (diffhe_lattice_pack_h16 produces both): 4 + 2 (nd - 1)
                                  instead of 4 nd bytes of coefficients per node and sample in the fp32-stored V-cycle.
                                  No kernel reads in front of (or behind) any array of this struct (ABI v7: the guard
                                  elements v6 asked for in front of vals32 / offdiag16 are gone) */
  const double* offdiag_scales; /* (Bv) device array, ABI v7: per-sample powers of two >= the sample's largest FREE-row
                                  diagonal entry (diffhe_lattice_max_diag), so samples of any magnitude share a batch;
                                  NULL = offdiag16 unused */
} diffhe_mg_level;

/* Option bits of `flags` (diffhe_lattice_pcg_solve; diffhe_ell_amg_pcg_solve reads FP32 and NO_FLOOR of the same word).
 * x, Ap and every dot product are fp64 whatever the bits, r is fp64 or an fp32 pair worth 48 bits (DIFFHE_PCG_RESID_FP64)
 * whose low half is dropped near the end of an energy-rule solve (DIFFHE_PCG_RESID_KEEP_LO);
 * bench.py records the word as solver_flags. */
#define DIFFHE_PCG_FP32 1              /* V-cycle and CG search directions stored in fp32 (arithmetic fp64 in registers) */
#define DIFFHE_PCG_FMG 2               /* start from a full-multigrid iterate instead of 0 */
#define DIFFHE_PCG_FMG_CYCLES_SHIFT 2  /* two bits: extra V-cycles per coarse level of that start (0..3) */
#define DIFFHE_PCG_NO_FLOOR 16         /* stop on `tol` alone; default: |r| <= max(tol |b|, 0.5 u |A_b| |x0_b|), u = 2^-53 */
#define DIFFHE_PCG_WARM 32             /* `x` holds an initial guess: start from x + FMG(b - A x) (with FMG) or from x */
#define DIFFHE_PCG_UNFUSED 64          /* fp32 cycle: four single-stage strip passes per level, not the fused two-stage ones */
#define DIFFHE_PCG_DENSE_SCALAR 128    /* fp32 cycle: coarsest dense solve by the scalar-load kernel, not the MFMA one */
#define DIFFHE_PCG_CLOSED_FP32_STEP 256 /* lattice closed by Dirichlet data, near-square cells: p.Ap in packed fp32 (cgstep2) */
#define DIFFHE_PCG_PRE2 512            /* fused PRE pass at two samples per lane (default: four where the batch allows) */
#define DIFFHE_PCG_RESID_FP64 (1 << 10) /* keep the CG residual as one fp64 vector + its fp32 copy where the default carries it
                                          as a pair of fp32 vectors (see diffhe_lattice_recompute_ap); A/B runs, tests */
#define DIFFHE_PCG_RESID_KEEP_LO (1 << 11) /* keep BOTH halves of that pair to the end of the solve; default: once every active
                                          sample's energy estimate is within 2^16 of the level the energy rule stops at, the
                                          residual update stops writing (then reading) the low half -- 16, then 12 instead of
                                          20 B per node and sample (status_host[3]); A/B runs, tests */
#define DIFFHE_PCG_TRUST_ITS_SHIFT (12) /* four bits, development and tests only: k > 0 trusts the energy rule for k iterations
                                          instead of the 10 (+ 1 per decade of tol_energy below 1e-11) of the default, 0 */
#define DIFFHE_PCG_SPLIT_START (1 << 16) /* keep the separate passes around the full-multigrid start of an fp32 solve with a
                                          batch-shared matrix: prolongation, then residual; conversion of the right-hand
                                          side, then its restriction; z0 copied into the direction ring by the first CG step.
                                          Default: each pair is one pass and z0 is written where p0 lives -- 4 B per node
                                          and sample less each, the same stored values bit for bit; A/B runs, tests */

/* Batched CG preconditioned by one multigrid V(nu,nu) cycle (weighted Jacobi with the
 * per-sweep damping factors omegas_host[0..nu-1] -- Chebyshev weights; post-smoothing runs
 * them in reverse so the cycle stays symmetric -- P1 transfers, n_coarse sweeps on the last
 * level; n_levels == 1 degenerates to a Jacobi polynomial).  Replaces torch.linalg.solve
 * (solver.py:174) forward and adjoint.
 *   levels   HOST array of n_levels descriptors (device pointers inside)
 *   Bv       Bp (matrix per sample) or 1 (shared); scale (Bp) or NULL: K_b = scale[b]*K on
 *            the free rows (one scalar kappa per sample, solver.py:88,139)
 *   flags    OR of the DIFFHE_PCG_* bits above
 *   tol      relative residual |r|_2 / |b|_2 per sample
 *   tol_energy  > 0: sample b ALSO stops once the estimated relative energy-norm error of its iterate,
 *            sqrt(r.z / u^T A u), is <= tol_energy.  r.z = r^T M^-1 r is the dot the CG needs for beta anyway;
 *            with the multigrid preconditioner M ~ A it equals e^T A e to the spectral equivalence of M and A;
 *            u^T A u ~ b.x0 of the full-multigrid start (r0.z0 from a zero start).  Nodal and per-element-gradient
 *            errors are what the parity tolerance is stated in, and the energy norm bounds both far more tightly
 *            than the residual does (1024^2, f = 1: relative residual 6e-9 <-> nodal error 6e-12).  0: off.
 *   err_est  (Bp) out or NULL: the last estimate per sample
 *   stop_rule (Bp) out or NULL (ABI v6): the rule that ended each sample -- 1 residual, 2 energy-norm estimate,
 *            0 neither (iteration cap reached, or the direct dense path where nothing iterates)
 *   b, x     (n, Bp) right-hand side / solution (x is read only with DIFFHE_PCG_WARM; otherwise the start is 0 / FMG(b))
 *   work     diffhe_lattice_pcg_workspace_doubles(...) doubles
 *   relres, iters, status_host: as diffhe_ell_cg_solve; status_host[3] = the residual updates of this solve that wrote no
 *            low half (forms F_RDROP / F_RSINGLE of csrc/lattice.h; 0 wherever the pair is not carried or is kept whole) */
long long diffhe_lattice_pcg_workspace_doubles(const diffhe_mg_level* levels, int n_levels, int Bp);
int diffhe_lattice_pcg_solve(const diffhe_mg_level* levels, int n_levels, int Bv, const double* scale,
                             const double* b, double* x, int Bp, double tol, double tol_energy, int max_iter, int nu,
                             int n_coarse, const double* omegas_host, int flags, double* work, double* relres,
                             double* err_est, int* iters, int* stop_rule, int* status_host, void* stream);
/* Opt-in timing of the fused CG-step kernel (the dominant one) inside diffhe_lattice_pcg_solve's own loop, for
 * bench.py's roofline entry: enable = 1 creates two HIP events (per calling thread, the only hidden state in the
 * library, and only in this mode) and resets the counters, 0 stops, < 0 only reads.  The events bracket each launch
 * on the solve's stream and are read after the loop's per-iteration synchronisation.  Returns the totals so far. */
int diffhe_lattice_pcg_profile(int enable, double* total_ms, long long* launches);
/* The same events exist for the other main kernels of an iteration (fine-level launches only); read-only access:
 *   id 0 fused CG step (full-work launches), 1 residual update r -= alpha Ap, 2 first two sweeps from 0,
 *      3 residual + restriction, 4 prolongation + sweep, 5 sweep.   enable / reset through diffhe_lattice_pcg_profile. */
int diffhe_lattice_kernel_profile(int id, double* total_ms, long long* launches);
/* Single kernels of that loop, exposed for timing/tests: y = A x (+ x.y block partials in
 * `part`, diffhe_lattice_blocks(n, Bp) * Bp doubles) and one damped-Jacobi sweep
 * xout = xin + omega (rhs - A xin)/D  (xin NULL = 0). */
int diffhe_lattice_blocks(int n, int Bp);
/* 2: the fp32 V-cycle of a batch-shared matrix runs the fused two-stage passes (pre-smoothing + residual + restriction;
 * prolongation + post-smoothing) with two samples per lane (one where the batch is no multiple of 128); DIFFHE_PCG_UNFUSED of
 * diffhe_lattice_pcg_solve switches them off per call (four single-stage strip passes per level).  Always 2 since the
 * development switches were retired.  With them, kernel-profile id 2 times the fused PRE pass (9 B per node and
 * sample), id 4 the fused POST pass (13 B), ids 3 and 5 see no launches. */
int diffhe_lattice_fused_passes(void);
/* 1: with a batch-shared matrix and fp32-stored search directions the PCG never stores A p -- the fused CG step keeps it
 * in registers for p.Ap (12 B per node and sample: z, p_old read, p written) and the residual update recomputes it from
 * the stored p (kernel-profile id 1).  On that path the residual is carried as the unevaluated sum of two fp32 vectors,
 * rs r = hi + lo with hi = (float)(rs r) the vector the V-cycle reads and rs the per-sample power of two of the fp32
 * copies: 48 bits (2^-48 relative per update), 20 B per node and sample (p read; hi, lo read and written) instead of the
 * 24 B of an fp64 r with its fp32 copy, which DIFFHE_PCG_RESID_FP64 keeps.  Where the energy rule is in force the low half
 * is dropped once every active sample is within 2^16 of its stop level: one update of 16 B, then 12 B (hi alone;
 * DIFFHE_PCG_RESID_KEEP_LO keeps the 20 B form).  Always 1 since the development
 * switches were retired; fp64 directions, per-sample matrices and the unfused loop still write A p (20 B) and read it
 * back in pcg_update_kernel (28 B). */
int diffhe_lattice_recompute_ap(void);
int diffhe_lattice_apply(const diffhe_mg_level* level, int Bv, const double* scale, const double* x, double* y,
                         double* part, int Bp, void* stream);
int diffhe_lattice_smooth(const diffhe_mg_level* level, int Bv, const double* scale, const double* rhs,
                          const double* xin, double* xout, double omega, int Bp, void* stream);
/* The fused CG step of diffhe_lattice_pcg_solve as a single launch (timing / tests):
 *   p_out = z + beta[b] p_in (first != 0: p_out = z);  x += alpha[b] p_in (skipped when first);
 *   Ap = A p_out;  part = block partials of p_out . Ap.   z, p_in and p_out are (n, Bp) fp32
 *   (z_fp32 != 0) or fp64: the search direction is stored in the precision of the preconditioner
 *   output; x, Ap and the dots are always fp64 and use the STORED p, so r = b - A x stays exact.
 * x == NULL: the iterate is left alone -- the form diffhe_lattice_pcg_solve launches since ABI v4: it keeps its
 *   directions in a ring of slots and forms x += sum_j alpha_j p_j when the ring is full / at the end, which takes
 *   the x read-modify-write (16 of 36 B per node) out of every iteration.
 * p_in and p_out must be different buffers (halo reads of p_in).  DIFFHE_E_TOOBIG below the
 * strip-kernel threshold. */
int diffhe_lattice_cg_step(const diffhe_mg_level* level, int Bv, const double* scale, const void* z, int z_fp32,
                           const void* p_in, void* p_out, double* x, const double* alpha, const double* beta,
                           int first, double* Ap, double* part, int Bp, void* stream);
/* out[b] = sum_i lam[i,b] * ((A x)[i,b] + add[i]): the dL/dkappa contraction of a batch-FACTORED
 * operator (K_b = kappa_b K_1: -lam^T K_1 u with u = x + g, add = K_1[free,bc] g), one pass over
 * x and lam instead of the element loop.  Returns DIFFHE_E_TOOBIG when the mesh/batch is below the
 * strip-kernel threshold (callers then use diffhe_p1_grad_kappa).  add (n) may be NULL;
 * part: diffhe_lattice_blocks(n, Bp) * Bp doubles; out (Bp). */
int diffhe_lattice_bilinear(const diffhe_mg_level* level, int Bv, const double* scale, const double* x,
                            const double* lam, const double* add, double* part, double* out, int Bp, void* stream);
/* y = mask ? 0 : (M x - sub_scale[b] * sub) for a batch-shared symmetric-diagonal matrix M (nd, n) of a
 * lattice mesh: the load vector F = M f minus the Dirichlet lift (solver.py:143-145, :166-169) and the
 * adjoint df = M^T lambda, without the general ELL pattern.  Arguments as diffhe_ell_spmv_shared. */
int diffhe_lattice_apply_shared(int nx, int ny, int nd, const double* vals, const double* x, const double* sub,
                                int sub_B, const double* sub_scale, const unsigned char* mask, double* y, int Bp,
                                void* stream);
/* dk[e, b] = - sum_{p,q} lambda[node_p, b] k0[p*3+q, e] (u[node_q, b] + g[node_q]) for every element of a LATTICE mesh
 * (FEMesh.rectangle connectivity) and every sample: the per-element gradient of diffhe_p1_grad_kappa as a strip pass
 * (each nodal value loaded once per wave instead of once per incident element).  k0 (9, m) unit-kappa element
 * matrices (k0_compact != 0, ABI v7: (9, 2), one per triangle orientation, as in diffhe_lattice_assemble_rows), lam / u
 * (n, Bp), g (n) or NULL, dk (m, Bp).  DIFFHE_E_TOOBIG for Bp < 64 (use diffhe_p1_grad_kappa). */
int diffhe_lattice_grad_kappa(int nx, int ny, const double* k0, int k0_compact, const double* lam, const double* u,
                              const double* g, double* dk, int Bp, void* stream);
/* Compact coefficient copies of a per-sample matrix for the fp32-stored V-cycle (diffhe_mg_level.vals32 / offdiag16):
 * diag32 (n, Bv) fp32, offdiag16 (nd - 1, n, Bv) fp16 of vals / offdiag_scales[b] (per-sample powers of two >= the
 * sample's max free-row diagonal, device array of Bv doubles); the diagonal absorbs the rounding differences of its row's
 * couplings, so the row sums -- what the smooth error modes see -- are those of `vals`.
 * flags (device int, may be NULL; the caller zeroes it): bit 0 is set when a non-zero coupling is smaller than 2^-19 of
 * its sample's scale -- fp16 keeps fewer than 5 bits there and flushes to 0 from 2^-25 on, which would leave rows with a
 * vanishing diagonal: the packed copies of a matrix with that much contrast INSIDE a sample must not be used (plain fp32
 * copies in vals32 have no such limit).  ABI v7. */
int diffhe_lattice_pack_h16(const diffhe_mg_level* level, int Bv, const double* offdiag_scales, float* diag32,
                            void* offdiag16, int* flags, void* stream);
/* out[b] = max over the FREE rows (is_bc == 0; identity rows carry 1.0 whatever kappa is) of the main diagonal of sample
 * b's level matrix, Bv doubles (zeroed inside).  ABI v7. */
int diffhe_lattice_max_diag(const diffhe_mg_level* level, int Bv, double* out, void* stream);
/* kappa of the coarse triangulation, arrays (m, Bv); sx, sy in {1, 2} = coarsening factor per direction.
 * Full coarsening: mean of the 4 children of each coarse triangle; semi: mean over the 2 covered fine cells. */
int diffhe_lattice_restrict_kappa(const double* kappa_fine, double* kappa_coarse, int nx_coarse, int ny_coarse,
                                  int sx, int sy, int Bv, void* stream);

/* dL/dkappa contraction (reverse of solver.py:89-92 / :137-140, Appendix A step 2):
 *   dk[e,b] = - sum_{p,q} lambda[elem_p,b] * k0[p*npe+q, e] * (u[elem_q,b] + g[elem_q])
 *   (u is the eliminated-system solution, 0 on Dirichlet nodes; g (n) adds the Dirichlet
 *   values back, may be NULL)
 *   dk_e (m, Bp) optional; dk_part (nblk, Bp) block partial sums over elements,
 *   dk_sum (Bp) their deterministic total. nblk = diffhe_grad_kappa_blocks(m, Bp). */
int diffhe_grad_kappa_blocks(int m, int Bp);
int diffhe_p1_grad_kappa(const int* elems, const double* k0, const double* lam, const double* u, const double* g,
                         int npe, int m, int Bp, double* dk_e, double* dk_part, double* dk_sum, void* stream);
/* The same contraction SUMMED OVER THE BATCH, dk[e] = sum_{b < B} dk[e,b] (m doubles): the gradient of a per-element
 * kappa field shared by all samples (reverse of solver.py:137-140 for kappa (m,)) -- what the RCCL gradient
 * all-reduce of BASELINE config 4 carries.  Fixed summation order (bitwise reproducible); the (m, Bp) per-sample
 * gradient is never materialised.  ABI v6. */
int diffhe_p1_grad_kappa_shared(const int* elems, const double* k0, const double* lam, const double* u, const double* g,
                                int npe, int m, int B, int Bp, double* dk, void* stream);

/* Anisotropic conductivity (csrc/aniso.hip): a symmetric tensor K per element in Voigt components, nc = 3 in 2D ordered
 * (xx, yy, xy), nc = 6 in 3D ordered (xx, yy, zz, yz, xz, xy); an off-diagonal component is one parameter for both
 * symmetric entries.  P1 triangles (dim 2) and tetrahedra (dim 3).  Added without a change of DIFFHE_ABI_VERSION: no
 * existing entry changed, and the binding resolves every symbol by name when it loads the library.
 *
 * Gradient-form element table: gtab (npe*dim, m), entry (p*dim + k, e) = d phi_p / d x_k up to the orientation sign of
 * the element (it cancels in every product of two gradients), vol (m) = area / volume; a degenerate element (the rules
 * of diffhe_p1_element_integrals) gets zeros in both. */
int diffhe_aniso_gradient_table(const double* coords, const int* elems, int dim, int n, int m, double* gtab, double* vol,
                                void* stream);
/* Row-gather assembly vals (W, n, Bv), lift (n, Bv) of K_e[p,q] = vol_e g_p^T K_e g_q over the lists of
 * diffhe_ell_assemble_rows, with its Dirichlet handling.  K component c of element e and sample b at
 * c*k_sc + e*k_se + b*k_sb (k_se = 0: one tensor for the mesh; k_sb = 0 with Bv = 1: one for the batch).  The pattern
 * must hold every coupling of the connectivity (no pruning of scalar-kappa zeros). */
int diffhe_aniso_assemble_rows(const double* gtab, const double* vol, int dim, const double* K, long long k_sc,
                               long long k_se, long long k_sb, const int* ent_ptr, const int* contrib, const int* cols,
                               const unsigned char* is_bc, const double* g, double* vals, double* lift, int n, int m,
                               int W, int Bv, void* stream);
/* dK_c[e,b] = -vol_e sym_c(grad lambda_eb (x) grad u_eb), grad lambda = sum_p lambda[elem_p, b] g_p, u likewise with
 * g (n, may be NULL) added on Dirichlet nodes; lam and u are (n, Bp).  dk_e optional: component c of (e, b) at
 * c*o_sc + e*o_se + b.  dk_part (diffhe_grad_kappa_blocks(m, Bp), nc, Bp) and dk_sum (nc, Bp), both or neither: the
 * sums over the elements per sample, two stages in a fixed order.  No atomics: bitwise reproducible. */
int diffhe_aniso_grad(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                      const double* u, const double* g, int n, int m, int Bp, double* dk_e, long long o_sc,
                      long long o_se, double* dk_part, double* dk_sum, void* stream);
/* The same gradient summed over the samples b < B in a fixed order: dk component c of element e at c*o_sc + e*o_se. */
int diffhe_aniso_grad_shared(const int* elems, const double* gtab, const double* vol, int dim, const double* lam,
                             const double* u, const double* g, int n, int m, int B, int Bp, double* dk, long long o_sc,
                             long long o_se, void* stream);

/* Shape derivative dL/dX of a P1 solve (1D segments, triangles, tetrahedra; ABI v8):
 *   grad[i, k] = sum over the elements e at node i of A_e [ (q_e - tr T_e) I + T_e + T_e^T ] grad phi_i,
 *   T_e = sum_{b<B} kappa[e*kse + b*ksb] grad u_eb (x) grad lambda_eb,   q_e = sum_{b<B} (load_eb - c lambda_eb . u_eb / (d+1)),
 *   load_eb = (sum_p lambda_pb)(sum_p f_pb) / (d+1)^2 in 2D / 3D, sum_p lambda_pb f_pb / 2 in 1D (the load maps of the
 *   solve), with A_e the element's length / area / volume; degenerate elements (the assembly's thresholds) add nothing.
 * coords (dim, n), elems (dim+1, m) as the element kernels take them.  u and lam (the adjoint, 0 on Dirichlet nodes) share
 * the strides: entry (i, b) at i*sn + b*sb -- (n, Bp) node-major: sn = Bp, sb = 1; the 1D chain's (B, n): sn = 1, sb = n;
 * g (n) is added to u (the eliminated-system solution) and may be NULL.  f (i, b) at i*fsn + b*fsb (fsb = 0: one forcing
 * for the batch), may be NULL.  inc_ptr (n+1) / inc: per node, the codes e*(dim+1) + p of its (element, local vertex)
 * pairs in a fixed order; work (m, (dim+1)*dim) doubles; grad (n, dim).  No atomics: bitwise reproducible. */
int diffhe_p1_shape_grad(const double* coords, const int* elems, int dim, int n, int m, int B, const double* u,
                         const double* g, const double* lam, long long sn, long long sb, const double* kappa,
                         long long kse, long long ksb, const double* f, long long fsn, long long fsb, double c,
                         const int* inc_ptr, const int* inc, double* work, double* grad, void* stream);

/* Per-sample Dirichlet data G_b (added entries of ABI v8; diffhe `dirichlet=`): the path kernels solve with HOMOGENEOUS Dirichlet data
 * and these four add what G_b changes, on the boundary band only (csrc/bc.hip).  K_b[i, j] = sum_{e ni i, j}
 * kappa[e*kse + b*ksb] k0[(p*npe + q)*m + e] is the UNREDUCED stiffness of sample b (kappa NULL: unit kappa); elems (npe, m)
 * and k0 (npe*npe, m) as the element kernels take them; d_slot (n): slot of a Dirichlet node in the ascending list of
 * Dirichlet nodes, -1 on free nodes.  G_b[j] (slot j) at G[j*gsj + b*gsb] (gsb = 0: one G for the batch).  Incidence
 * lists: per row, the codes e*npe + p of its (element, local node) pairs in a fixed order.  No atomics: bitwise
 * reproducible.  Only samples b < B are touched.
 * lift:    rhs[rows[r]*rsn + b*rsb] -= sum_{(e, p) of row r} kappa_eb sum_{q: Dirichlet} k0_e[p, q] G_b[slot(q)]
 *          (rows: the free nodes with a Dirichlet neighbour; row_inc: their pairs in elements that touch D).
 * grad:    out[j*osj + b*osb] = gbar[d_idx[j]*gsn + b*gsb] - (K_b lam_b)_{d_idx[j]}   (gbar may be NULL: 0), with lam
 *          (0 on Dirichlet nodes; only its free entries are read) at lam[i*lsn + b*lsb] and d_inc every pair of each
 *          Dirichlet node; dots (n_d, B) or NULL: dots[j*B + b] = G_b[j] (K_1 lam_b)_{d_idx[j]} (unit kappa).
 * scatter: u[d_idx[j]*usn + b*usb] = G_b[j].
 * grad_kappa: dk[e*dse + b*dsb] -= sum_{p free, q Dirichlet} lam_b[p] k0_e[p, q] G_b[slot(q)] on the elements band_elems
 *          that touch a Dirichlet node; shared != 0: dk[e*dse] -= the same summed over b < B. */
int diffhe_bc_lift(const int* elems, int npe, int m, const double* k0, const double* kappa, long long kse,
                   long long ksb, const int* d_slot, const double* G, long long gsj, long long gsb, const int* rows,
                   const int* row_ptr, const int* row_inc, int n_rows, double* rhs, long long rsn, long long rsb, int B,
                   void* stream);
int diffhe_bc_grad(const int* elems, int npe, int m, const double* k0, const double* kappa, long long kse,
                   long long ksb, const int* d_slot, const int* d_idx, const int* d_ptr, const int* d_inc, int n_d,
                   const double* lam, long long lsn, long long lsb, const double* gbar, long long gsn, long long gsb,
                   double* out, long long osj, long long osb, const double* G, long long Gsj, long long Gsb,
                   double* dots, int B, void* stream);
int diffhe_bc_scatter(const int* d_idx, int n_d, const double* G, long long gsj, long long gsb, double* u,
                      long long usn, long long usb, int B, void* stream);
int diffhe_bc_grad_kappa(const int* elems, int npe, int m, const double* k0, const int* d_slot, const int* band_elems,
                         int n_be, const double* lam, long long lsn, long long lsb, const double* G, long long gsj,
                         long long gsb, double* dk, long long dse, long long dsb, int shared, int B, void* stream);

/* Robin (convective) and flux boundary conditions, kappa du/dn + h_F (u - uinf_F) = q_F on boundary facets (csrc/robin.hip;
 * diffhe.robin).  Added without a change of DIFFHE_ABI_VERSION, like the aniso entries: no existing entry changed.  A facet
 * has d nodes (1: an end point of a chain, 2: an edge, 3: a face of a tetrahedron), fac (d, nF); its consistent P1 mass is
 * M_F[p, q] = area[F] (1 + delta_pq) / (d (d + 1)).  h, uinf, q of facet F and sample b sit at F*sf + b*sb of their array
 * (sf = 0: one value for all facets, sb = 0: one for the batch; a NULL array is all zeros).  No atomics: bitwise
 * reproducible.
 * facet_table: area[F] = 1 (d = 1), the edge length (d = 2; 0 below 1e-15) or the triangle area (d = 3; 0 when
 *   |a x b| <= 1e-12 l^2, l the longer of the edges a, b from the first node); coords (dim, n) with dim = d.
 * assemble: for every band row r (a FREE node rows[r] on a facet) and its entries t in [row_ptr[r], row_ptr[r+1]), code
 *   ent_code[t] = F*16 + p*4 + c (p the row's local index in F, c the column's): vals[(ent_slot[t]*n + row)*Bv + b] +=
 *   h_Fb M_F[p, c], or with ent_slot[t] < 0 (Dirichlet column) rhs -= h_Fb M_F[p, c] g[node c]; entries with p == c also
 *   add (h_Fb uinf_Fb + q_Fb) area[F] / d to rhs[row*Bp + b].  vals (W, n, Bv) as the ELL assembly left them, rhs
 *   (n, Bp); Bv = 1 needs a batch-shared h.  Padding samples B <= b < Bp: h = 1 where h comes per sample, no load.
 * grad: lam, u (n, Bp), g (n) or NULL added to u; with s = (area[F] / d) sum_p lam_p:  dq = s,  du = h_Fb s,
 *   dh = uinf_Fb s - lam_F^T M_F u_F.  Each output may be NULL; (F, b) is written at F*of + b*ob, and ob = 0 asks for the
 *   sum over the samples b < B (fixed order) at F*of.
 * sum_facets: out[b] = sum_F src[F*B + b] in two fixed-order stages; part holds diffhe_robin_sum_blocks(nF) * B doubles. */
int diffhe_robin_facet_table(const double* coords, const int* fac, int dim, int n, int nF, double* area, void* stream);
int diffhe_robin_assemble(const int* fac, int d, int nF, const double* area, const int* rows, const int* row_ptr,
                          const int* ent_code, const int* ent_slot, int n_rows, const double* g, const double* h,
                          long long hsf, long long hsb, const double* uinf, long long usf, long long usb, const double* q,
                          long long qsf, long long qsb, double* vals, double* rhs, int n, int Bv, int B, int Bp,
                          void* stream);
int diffhe_robin_grad(const int* fac, int d, int nF, const double* area, const double* lam, const double* u,
                      const double* g, int B, int Bp, const double* h, long long hsf, long long hsb, const double* uinf,
                      long long usf, long long usb, double* dh, long long dhf, long long dhb, double* du, long long duf,
                      long long dub, double* dq, long long dqf, long long dqb, void* stream);
int diffhe_robin_sum_blocks(int nF);
int diffhe_robin_sum_facets(const double* src, int nF, int B, double* part, double* out, void* stream);

/* Coefficient-aware aggregation hierarchy of the general path: its set-up passes (csrc/coarsen.hip; diffhe.amg).  Added
 * without a change of DIFFHE_ABI_VERSION, like the aniso and robin entries: no existing entry changed.  vals (W, n, Bv) are
 * the assembled ELL values of a call (slot 0 = diagonal, padding slots point at the row itself and hold 0).  No atomics:
 * bitwise reproducible.
 * sample_scales: out[b] = sum over the rows i with is_bc[i] == 0 (is_bc NULL: all rows) of vals[i*Bv + b], the diagonal,
 *   in two fixed-order stages; part holds ceil(n / DIFFHE_ELL_SCALE_CHUNK) * Bv doubles.
 * mean_operator: out[k*n + i] = (sum_{b < B} vals[(k*n + i)*Bv + b] * weight[b]) / B -- with weight[b] = 1 / (mean
 *   free-row diagonal of sample b) the representative operator of the batch; the samples b >= B (padding) are not read.
 *   Bv == 1 (B == 1): a scaled copy.
 * strength_filter: on one matrix abar (W, n), W <= 64.  c_ij = max(-a_ij, 0) / sqrt(a_ii a_jj); slot k of row i (column
 *   j) is STRONG when c_ij > 0, c_ij >= theta * max_k c_ik and, looked up in row j, c_ji > 0, c_ji >= theta * max_l c_jl.
 *   strong_cols[k*n + i] = j on strong slots, i elsewhere (the graph diffhe.amg.aggregate reads); filt: abar with the
 *   weak off-diagonals set to 0 and added to the diagonal in slot order (row sums kept). */
#define DIFFHE_ELL_SCALE_CHUNK 256
int diffhe_ell_sample_scales(const double* vals, const unsigned char* is_bc, int n, int Bv, double* part, double* out,
                             void* stream);
int diffhe_ell_mean_operator(const double* vals, const double* weight, int n, int W, int Bv, int B, double* out,
                             void* stream);
int diffhe_ell_strength_filter(const double* abar, const int* cols, int n, int W, double theta, int* strong_cols,
                               double* filt, void* stream);

/* Block machinery of the batched eigensolver, K phi = lambda M_L phi per sample (csrc/eigen.hip; diffhe.eigen).  Added
 * without a change of DIFFHE_ABI_VERSION, like the aniso, robin and coarsen entries: no existing entry changed.  A block of
 * p <= 16 vectors is (p, n, Bp): column c is an (n, Bp) array at c * n * Bp.  Small per-sample matrices are (p, p, Bp), entry
 * (r, c) of sample b at (r*p + c)*Bp + b; symmetric ones are packed by the rows of their upper triangle,
 * q(i, j) = i*p - i*(i-1)/2 + (j - i) for i <= j, as (p(p+1)/2, Bp).  Every sum over the nodes runs in two fixed-order
 * stages over diffhe_eig_gram_blocks(n, Bp) block partials; no atomics: bitwise reproducible.
 * gram:     GA[q(i,j)] = y_i . (AY)_j, GM[q(i,j)] = y_i . (mass * y_j) over the rows with is_bc == 0 (is_bc NULL: all rows);
 *           part holds blocks * p(p+1) * Bp doubles.  The (i, j) pairs are tiled 4 x 4 over the grid: Y and AY are read
 *           (2 d + 3 o) / (2 t) times, t = ceil(p/4) tiles, d = t diagonal and o = t(t-1)/2 off-diagonal pairs (1.75 at p = 8,
 *           3.25 at p = 16).
 * ritz:     one sample per lane: Cholesky GM = L L^T, cyclic Jacobi (at most `sweeps` sweeps) on L^-1 GA L^-T, eigenvalues
 *           ascending in theta (p, Bp), C (p, p, Bp) = L^-T V so that C^T GA C = diag(theta), C^T GM C = I.  work: 2 p p Bp
 *           doubles.  flag[b] = 1 where GM is not positive definite or an input is not finite: C = I and theta = 0 there.
 * rotate:   X = Y C, AX = AY C, and from the same registers MX = mass * X and R = theta * MX - AX (each of the two may be
 *           NULL; theta is read for R only).  The outputs must not alias the inputs.  C is staged in LDS, at most 128 / p
 *           columns per pass: p > 11 re-reads Y and AY once more.
 * residual: rho[c, b] = sqrt(sum_i R[c, i, b]^2 / mass_i) / |theta[c, b]| (1e300 where theta is 0); part: blocks * p * Bp.
 * fix_sign: in place on the first k columns: column c of sample b is negated unless sum_i mass_i x_i > 0 -- where that sum
 *           is below 1e-8 in magnitude, unless its entry of largest magnitude is positive.  sgn (k, Bp) receives the
 *           factors; part: blocks * 2 k * Bp doubles. */
int diffhe_eig_gram_blocks(int n, int Bp);
int diffhe_eig_gram(const double* Y, const double* AY, const double* mass, const unsigned char* is_bc, int p, int n,
                    int Bp, double* part, double* GA, double* GM, void* stream);
int diffhe_eig_ritz(const double* GA, const double* GM, int p, int Bp, int sweeps, double* work, double* C, double* theta,
                    int* flag, void* stream);
int diffhe_eig_rotate(const double* Y, const double* AY, const double* C, const double* theta, const double* mass, int p,
                      int n, int Bp, double* X, double* AX, double* MX, double* R, void* stream);
int diffhe_eig_residual(const double* R, const double* theta, const double* mass, int p, int n, int Bp, double* part,
                        double* rho, void* stream);
int diffhe_eig_fix_sign(double* X, const double* mass, int k, int n, int Bp, double* part, double* sgn, void* stream);

/* Layout changes between the API's (B, n) and the solver's (n, Bp).
 * to_node_major: dst[i*Bp + b] = src[b*ld + i] (b < B), 0 for padding samples and
 *   where zero_mask[i] != 0 (zero_mask may be NULL; src row stride ld = 0 broadcasts).
 * to_sample_major: dst[b*ld + i] = src[i*Bp + b] + add[i] (add may be NULL). */
int diffhe_to_node_major(const double* src, long long ld, const unsigned char* zero_mask, double* dst, int n, int B,
                         int Bp, void* stream);
int diffhe_to_sample_major(const double* src, const double* add, double* dst, long long ld, int n, int B, int Bp,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFHE_HIP_H */
