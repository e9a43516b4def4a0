"""diffhe -- MI355X-native differentiable P1-FEM solve path.

Drop-in for the public surface of danieleschmidt/DiffFE-Physics-Lab
(reference diffhe/__init__.py:6-12): same names, same call semantics; the solve
itself runs in hand-written HIP kernels (libdiffhe_hip.so, include/diffhe_hip.h).
Extras that have no reference counterpart live in submodules only
(`diffhe.distributed`: batch sharding over ranks; `diffhe.heat`: time stepping of the heat equation, the
reference's roadmap item; `diffhe.tet3d`: `DifferentiableFESolver3D`, solves on 3D tetrahedral meshes such as
`FEMesh.box`; `diffhe.shape`: `ShapeDifferentiableFESolver`, gradients with respect to the node coordinates, also
exported here; `diffhe.dirichlet`: the adjoint step behind `forward(..., dirichlet=)`, per-sample Dirichlet values with
gradients; `diffhe.aniso`: `AnisotropicFESolver`, solves with a conductivity tensor per element and its gradient, also
exported here; `diffhe.robin`: `RobinFESolver`, Robin (convective) and flux boundary conditions on boundary facets with
gradients to the film coefficient, the ambient value and the flux, also exported here; `diffhe.eigen`: `EigenFESolver`,
the smallest eigenpairs of K phi = lambda M_L phi per sample with d lambda / d kappa, also exported here;
`diffhe.elastic`: `ElasticFESolver`, linear elasticity on P1 triangles and tetrahedra -- the first vector-valued problem,
d displacement components per node -- with gradients to a Young's modulus per element, the body force and the nodal
load, also exported here (its kernels are declared in include/diffhe_elastic.h), and the ONE call pipeline of the elastic
family (`_ElasticSolve.forward` / `adjoint` with hooks, the hierarchy choice, the call builder, the shared plumbing of
the solve ops, the shared construction of the public solvers) that the other elastic modules build on;
`diffhe.elastic_stress`, re-exported by `diffhe.elastic`: its `stress` / `von_mises` with
gradients to u and E and `pnorm` (kernels declared in include/diffhe_stress.h), and its eigenstrain (initial strain:
thermal expansion, swelling, pre-stress) -- `eigenstrain_load`, `eigenstrain=` on the solve and on the stress methods,
with gradients to eps0 and E, and the torch helpers `thermal_strain` / `element_mean` that carry the temperature of a
heat solve to it (kernels declared in include/diffhe_eigenstrain.h); `diffhe.modal`: `ElasticEigenSolver`, the vibration
modes K(E) phi = lambda M(rho) phi of elastic bodies per sample with d lambda / dE and d lambda / d rho, also exported
here (kernels declared in include/diffhe_modal.h); `diffhe.elastic_shape`: `ShapeElasticFESolver`, `ElasticFESolver`
that also returns dL/dX for the node coordinates of the solve and of its `stress` / `von_mises`, from the same single
adjoint solve -- shape design of elastic bodies -- also exported here (kernels declared in
include/diffhe_elastic_shape.h); `diffhe.elastic_aniso`: `AnisotropicElasticFESolver`, `ElasticFESolver` with a stiffness
tensor per element and sample in place of (E, nu) and its gradient dL/dC -- laminates, orthotropic and cubic materials,
gradients to Poisson's ratio -- with the torch helpers that build and rotate such tensors, also exported here (kernels
declared in include/diffhe_elastic_aniso.h), with `diffhe.elastic_aniso_stress`: the stress sigma = C eps(u) of such a solve
and the fused quadratic failure index phi = q . sigma + sigma . Q sigma (Tsai-Wu, Tsai-Hill, von Mises as a quadratic form),
differentiable in u, C and the criterion (`tensor_stress`, `failure_index` on the solver; the criterion helpers `tsai_wu`,
`tsai_hill`, `quadratic`, `split`, `von_mises_criterion`, `rotated_criterion`, also exported here; kernels declared in
include/diffhe_elastic_aniso_stress.h); `diffhe.elastic_facets`: `TractionElasticFESolver`, `ElasticFESolver` with
tractions, pressure and an elastic (Winkler) foundation on boundary facets, per facet and sample, and their gradients,
also exported here (kernels declared in include/diffhe_elastic_facets.h); `diffhe.filters`: `DensityFilter`, the
mesh-independent density filter with a physical radius on the elements of any P1 mesh and its exact adjoint, also exported
here, and the tanh projection `heaviside` -- the regularisation of a design in front of the solvers (kernels declared in
include/diffhe_filter.h); `diffhe.sampling`: `PointSampler`, nodal fields sampled at arbitrary points of any P1 mesh, their
spatial gradient there and the exact transposes -- readings of sensors that do not sit on nodes, and the transfer of a
field from one mesh to another -- also exported here (kernels declared in include/diffhe_sample.h); `diffhe.hyperelastic`:
`HyperelasticFESolver`, the large-displacement counterpart of `ElasticFESolver` -- compressible Neo-Hookean material at
finite strain in plane strain and 3D, Newton's method with load steps and a per-sample line search, dL/dE, dL/df and
dL/dload from one adjoint solve with the final tangent -- also exported here (kernels declared in
include/diffhe_hyperelastic.h), with `diffhe.hyper_stress`: the Cauchy stress, its von Mises stress and the strain-energy
density of such a solve, differentiable in u and E (`cauchy_stress`, `cauchy_von_mises`, `energy_density` on the solver;
kernels declared in include/diffhe_hyper_stress.h); `diffhe.buckling`: `LinearBucklingSolver`, the critical load factors
(K(E) + lambda K_G(sigma0)) phi = 0 of elastic bodies per sample and their modes -- the fourth classical structural design
problem next to compliance, stress and eigenfrequencies -- with d lambda / dE and d lambda / d sigma0, the prestress taken
from a solve of its own or given, and `aggregate`, the smooth lower bound of the smallest factor, also exported here
(kernels declared in include/diffhe_buckling.h); `diffhe._hip`: the ctypes binding).
"""
from . import (aniso as _aniso, buckling as _buckling, eigen as _eigen, elastic as _elastic, elastic_aniso as _elastic_aniso, elastic_aniso_stress as _elastic_aniso_stress, elastic_facets as _elastic_facets, elastic_shape as _elastic_shape, filters as _filters, hyperelastic as _hyperelastic, loss as _loss, mesh as _mesh, modal as _modal, neural as _neural, robin as _robin, sampling as _sampling, shape as _shape,
               solver as _solver)

FEMesh = _mesh.FEMesh
DifferentiableFESolver = _solver.DifferentiableFESolver
PhysicsLoss = _loss.PhysicsLoss
NeuralPDE = _neural.NeuralPDE
ShapeDifferentiableFESolver = _shape.ShapeDifferentiableFESolver
AnisotropicFESolver = _aniso.AnisotropicFESolver
RobinFESolver = _robin.RobinFESolver
EigenFESolver = _eigen.EigenFESolver
ElasticFESolver = _elastic.ElasticFESolver
ElasticEigenSolver = _modal.ElasticEigenSolver
ShapeElasticFESolver = _elastic_shape.ShapeElasticFESolver
AnisotropicElasticFESolver = _elastic_aniso.AnisotropicElasticFESolver
TractionElasticFESolver = _elastic_facets.TractionElasticFESolver
DensityFilter = _filters.DensityFilter
PointSampler = _sampling.PointSampler
HyperelasticFESolver = _hyperelastic.HyperelasticFESolver
LinearBucklingSolver = _buckling.LinearBucklingSolver
tsai_wu, tsai_hill = _elastic_aniso_stress.tsai_wu, _elastic_aniso_stress.tsai_hill
quadratic, split = _elastic_aniso_stress.quadratic, _elastic_aniso_stress.split
von_mises_criterion = _elastic_aniso_stress.von_mises_criterion
rotated_criterion = _elastic_aniso_stress.rotated_criterion

__all__ = ("FEMesh", "DifferentiableFESolver", "PhysicsLoss", "NeuralPDE", "ShapeDifferentiableFESolver",
           "AnisotropicFESolver", "RobinFESolver", "EigenFESolver", "ElasticFESolver", "ElasticEigenSolver",
           "ShapeElasticFESolver", "AnisotropicElasticFESolver", "TractionElasticFESolver", "DensityFilter",
           "PointSampler", "HyperelasticFESolver", "LinearBucklingSolver", "tsai_wu", "tsai_hill", "quadratic", "split", "von_mises_criterion",
           "rotated_criterion")
__version__ = "0.1.0"          # tracks the reference release this surface mirrors
