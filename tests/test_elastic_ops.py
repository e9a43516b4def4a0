"""The op surface of the elastic family (`diffhe.elastic`, `elastic_stress`, `elastic_shape`, `elastic_aniso`,
`elastic_facets`, `modal`): the schema of every custom op, pinned, and the lifetime of the solver behind the stress and
eigenstrain ops -- the registry of `diffhe.solver` holds a solver weakly, so the autograd graph of an op that looks its
solver up again in backward has to keep it alive.
"""
import gc

import pytest
import torch

import diffhe  # noqa: F401  (registers the ops)
from diffhe import ElasticFESolver, FEMesh, ShapeElasticFESolver

T64 = torch.float64
DEV = "cuda:0"

SCHEMAS = {
    "elastic_solve": "diffhe::elastic_solve(Tensor E, Tensor f, Tensor load, SymInt handle, bool save, bool node_major) "
                     "-> (Tensor, Tensor)",
    "elastic_solve_backward": "diffhe::elastic_solve_backward(Tensor gbar, Tensor token, bool need_e, bool need_f, bool "
                              "need_load, Tensor e_like, Tensor f_like, Tensor load_like) -> (Tensor, Tensor, Tensor)",
    "elastic_solve_shape": "diffhe::elastic_solve_shape(Tensor E, Tensor f, Tensor load, Tensor nodes, SymInt "
                           "nodes_version, SymInt handle, bool node_major) -> (Tensor, Tensor)",
    "elastic_solve_shape_backward": "diffhe::elastic_solve_shape_backward(Tensor gbar, Tensor token, bool need_e, bool "
                                    "need_f, bool need_load, bool need_x, Tensor e_like, Tensor f_like, Tensor load_like, "
                                    "Tensor nodes_like) -> (Tensor, Tensor, Tensor, Tensor)",
    "elastic_aniso_solve": "diffhe::elastic_aniso_solve(Tensor C, Tensor f, Tensor load, SymInt handle, bool save, bool "
                           "node_major) -> (Tensor, Tensor)",
    "elastic_aniso_solve_backward": "diffhe::elastic_aniso_solve_backward(Tensor gbar, Tensor token, bool need_c, bool "
                                    "need_f, bool need_load, Tensor c_like, Tensor f_like, Tensor load_like) -> (Tensor, "
                                    "Tensor, Tensor)",
    "elastic_facet_solve": "diffhe::elastic_facet_solve(Tensor E, Tensor f, Tensor load, Tensor traction, Tensor pressure, "
                           "Tensor k_normal, Tensor k_tangent, SymInt handle, bool save, bool node_major) -> (Tensor, "
                           "Tensor)",
    "elastic_facet_solve_backward": "diffhe::elastic_facet_solve_backward(Tensor gbar, Tensor token, bool need_e, bool "
                                    "need_f, bool need_load, bool need_t, bool need_p, bool need_kn, bool need_kt, Tensor "
                                    "e_like, Tensor f_like, Tensor load_like, Tensor t_like, Tensor p_like, Tensor kn_like, "
                                    "Tensor kt_like) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "elastic_stress": "diffhe::elastic_stress(Tensor u, Tensor E, SymInt handle, bool node_major, bool want_sigma, bool "
                      "want_vm) -> (Tensor, Tensor)",
    "elastic_stress_backward": "diffhe::elastic_stress_backward(Tensor sigma_bar, Tensor vm_bar, Tensor u, Tensor E, SymInt "
                               "handle, bool node_major, bool need_u, bool need_e) -> (Tensor, Tensor)",
    "elastic_stress_eigen": "diffhe::elastic_stress_eigen(Tensor u, Tensor E, Tensor eps0, SymInt handle, bool node_major, "
                            "bool want_sigma, bool want_vm) -> (Tensor, Tensor)",
    "elastic_stress_eigen_backward": "diffhe::elastic_stress_eigen_backward(Tensor sigma_bar, Tensor vm_bar, Tensor u, "
                                     "Tensor E, Tensor eps0, SymInt handle, bool node_major, bool need_u, bool need_e, bool "
                                     "need_z) -> (Tensor, Tensor, Tensor)",
    "elastic_stress_shape": "diffhe::elastic_stress_shape(Tensor u, Tensor E, Tensor nodes, SymInt nodes_version, SymInt "
                            "handle, bool node_major, bool want_sigma, bool want_vm) -> (Tensor, Tensor)",
    "elastic_stress_shape_backward": "diffhe::elastic_stress_shape_backward(Tensor sigma_bar, Tensor vm_bar, Tensor u, "
                                     "Tensor E, Tensor nodes, SymInt handle, bool node_major, bool need_u, bool need_e, bool "
                                     "need_x) -> (Tensor, Tensor, Tensor)",
    "eigenstrain_load": "diffhe::eigenstrain_load(Tensor eps0, Tensor E, SymInt handle, bool node_major, SymInt B_hint) -> "
                        "Tensor",
    "eigenstrain_load_backward": "diffhe::eigenstrain_load_backward(Tensor gbar, Tensor eps0, Tensor E, SymInt handle, bool "
                                 "node_major, SymInt B_hint, bool need_z, bool need_e) -> (Tensor, Tensor)",
    "modal_solve": "diffhe::modal_solve(Tensor E, Tensor rho, Tensor? x0, SymInt handle, SymInt batch, bool node_layout, "
                   "bool save) -> (Tensor, Tensor, Tensor)",
    "modal_solve_backward": "diffhe::modal_solve_backward(Tensor glam, Tensor token, bool need_e, bool need_r, Tensor "
                            "e_like, Tensor r_like) -> (Tensor, Tensor)",
}


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_op_schema_is_pinned(name):
    assert str(getattr(torch.ops.diffhe, name).default._schema) == SCHEMAS[name]


def test_eighteen_ops_are_pinned():
    assert len(SCHEMAS) == 18


# ------------------------------------------------------------------------------------------------
# GPU: the graph of a stress or eigenstrain evaluation keeps its solver alive
# ------------------------------------------------------------------------------------------------
def _rand(shape, seed, lo=-1.0, hi=1.0):
    return lo + (hi - lo) * torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=T64)


def _lifetime_case(kind):
    """-> (make solver, evaluate(solver, leaves) -> output, make leaves) on rectangle(2, 2): 3 x 3 nodes, 8 triangles."""
    base = FEMesh.rectangle(2, 2)
    n, m, B = base.n_nodes, base.n_elements, 2
    assert (n, m) == (9, 8)
    E = _rand((B, m), 1, 0.5, 2.0).to(DEV)
    u0, eps0 = _rand((B, n, 2), 2), _rand((B, m, 3), 3, -1e-2, 1e-2)
    leaf = lambda t: t.clone().to(DEV).requires_grad_(True)  # noqa: E731
    if kind == "von_mises":
        return (lambda: ElasticFESolver(base, E, device=DEV), lambda s, x: s.von_mises(x[0]), lambda: [leaf(u0)])
    if kind == "von_mises_eigenstrain":
        return (lambda: ElasticFESolver(base, E, device=DEV), lambda s, x: s.von_mises(x[0], eigenstrain=x[1]),
                lambda: [leaf(u0), leaf(eps0)])
    if kind == "eigenstrain_load":
        return (lambda: ElasticFESolver(base, E, device=DEV), lambda s, x: s.eigenstrain_load(x[0]), lambda: [leaf(eps0)])

    def moving():
        X = base.nodes.to(T64).clone().requires_grad_(True)
        return ShapeElasticFESolver(FEMesh(nodes=X, elements=base.elements, dirichlet_nodes=base.dirichlet_nodes), E,
                                    device=DEV)
    return moving, lambda s, x: s.von_mises(x[0]), lambda: [leaf(u0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["von_mises", "von_mises_eigenstrain", "eigenstrain_load", "shape_von_mises"])
def test_backward_after_the_solver_is_dropped(kind):
    """A detached u (or eps0) that requires grad, the output taken, the solver deleted and collected, then backward: the
    gradient is the one a solver that stays alive gives, bit for bit."""
    make, evaluate, leaves = _lifetime_case(kind)
    alive, ref = make(), leaves()
    evaluate(alive, ref).sum().backward()
    moving_ref = alive.mesh.nodes.grad.clone() if kind == "shape_von_mises" else None
    solver, x = make(), leaves()
    out = evaluate(solver, x)
    nodes = solver.mesh.nodes
    del solver
    gc.collect()
    out.sum().backward()
    for got, want in zip(x, ref):
        assert got.grad is not None and torch.equal(got.grad, want.grad)
    if moving_ref is not None:
        assert torch.equal(nodes.grad, moving_ref)
