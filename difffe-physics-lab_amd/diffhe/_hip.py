"""ctypes binding of libdiffhe_hip.so (include/diffhe_hip.h, include/diffhe_elastic.h, include/diffhe_stress.h,
include/diffhe_eigenstrain.h, include/diffhe_modal.h, include/diffhe_elastic_shape.h, include/diffhe_elastic_aniso.h,
include/diffhe_elastic_facets.h, include/diffhe_filter.h, include/diffhe_sample.h, include/diffhe_hyperelastic.h,
include/diffhe_hyper_stress.h, include/diffhe_elastic_aniso_stress.h, include/diffhe_buckling.h, include/diffhe_lobpcg.h).

The library is built in-tree by `__graft_entry__.build()` /
`make -C difffe-physics-lab_amd/csrc`.  There is NO fallback: if the library or a
GPU is missing every solve raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DIFFHE_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libdiffhe_hip.so"))

_P, _I, _L, _D = C.c_void_p, C.c_int, C.c_longlong, C.c_double     # _P: struct members (no from_param there)
ABI_VERSION = 8     # DIFFHE_ABI_VERSION of include/diffhe_hip.h this binding was written against


class MgLevel(C.Structure):
    """struct diffhe_mg_level (include/diffhe_hip.h)."""
    _fields_ = [("nx", _I), ("ny", _I), ("nd", _I), ("reserved", _I), ("vals", _P), ("is_bc", _P), ("vals32", _P),
                ("dense_inv", _P), ("shift", _P), ("rdiag32", _P), ("mask32", _P), ("offdiag16", _P), ("offdiag_scales", _P)]


_LV = C.POINTER(MgLevel)


class AmgLevel(C.Structure):
    """struct diffhe_amg_level (include/diffhe_hip.h)."""
    _fields_ = [("n", _I), ("W", _I), ("vals", _P), ("cols", _P), ("agg", _P), ("agg_ptr", _P), ("agg_members", _P),
                ("vals32", _P), ("agg_weights", _P), ("p_cols", _P), ("p_vals", _P), ("p_width", _I), ("reserved", _I),
                ("dense_inv", _P)]


_AV = C.POINTER(AmgLevel)


class _Ptr:
    """Pointer argtype of one element type: None -> NULL, a tensor of that dtype -> its data_ptr(), a c_void_p or an
    int address -> itself, unchecked.  Any other tensor is refused (ctypes.ArgumentError) before the call is made."""
    dtype = None        # None: void*, any tensor

    @classmethod
    def from_param(cls, v):
        if v is None:
            return None
        if type(v) is int:          # a stream or a raw address: wrapped, ctypes would pass a bare int as a C int
            return C.c_void_p(v)
        if isinstance(v, torch.Tensor):
            if v.dtype is not cls.dtype and cls.dtype is not None:
                raise TypeError(f"{v.dtype} tensor where the header declares {cls.elem}*")
            return C.c_void_p(v.data_ptr())
        if isinstance(v, C.c_void_p):
            return v
        raise TypeError(f"{type(v).__name__} where the header declares {cls.elem}*")


def _ptr_type(elem: str, dtype) -> type:
    return type("_Ptr_" + elem.replace(" ", "_"), (_Ptr,), {"elem": elem, "dtype": dtype})


_PD, _PF = _ptr_type("double", torch.float64), _ptr_type("float", torch.float32)
_PI, _PL = _ptr_type("int", torch.int32), _ptr_type("long long", torch.int64)
_PB, _PV = _ptr_type("unsigned char", torch.uint8), _ptr_type("void", None)


class _S:
    """Marker restype: a C int that is a DIFFHE_OK / DIFFHE_E_* status -- `lib()` binds it as c_int with `_errcheck`."""


# name -> (restype, argtypes); must list every symbol of include/diffhe_hip.h with the header's types
# (tests/test_abi.py).  Plain _I where an int is a value, where the caller reads a status itself (diffhe_lattice_bilinear)
# and on the profile / traffic accessors, whose status callers have always been free to ignore.
SIGNATURES = {
    "diffhe_abi_version": (_I, []),
    "diffhe_status_string": (C.c_char_p, [_I]),
    "diffhe_last_hip_error": (C.c_char_p, []),
    "diffhe_traffic_account": (_I, [_I, C.POINTER(_D), C.POINTER(_L)]),
    "diffhe_chain1d_stage_doubles": (_L, [_I, _I, _I, _I]),
    "diffhe_chain1d_solve": (_S, [_PD, _PD, _L, _L, _PD, _L, _PI, _I, _PD, _PD, _L, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_chain1d_adjoint": (_S, [_PD, _PD, _L, _L, _PD, _L, _PD, _L, _PI, _I, _PD, _L, _PD, _L, _PD, _I, _I, _I, _I,
                                    _PD, _PV]),
    "diffhe_p1_element_integrals": (_S, [_PD, _PI, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_ell_assemble_rows": (_S, [_PD, _PD, _L, _L, _PI, _PI, _PI, _PI, _PB, _PD, _PD, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_lattice_assemble_rows": (_S, [_PD, _I, _PD, _L, _L, _PB, _PD, _PD, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_ell_assemble_rows_ref": (_S, [_PD, _PD, _PD, _L, _L, _PI, _PI, _PI, _PI, _PB, _PD, _PD, _PD, _I, _I, _I, _I,
                                          _PV]),
    "diffhe_ell_assemble_atomic": (_S, [_PD, _PI, _I, _PD, _L, _L, _PI, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_ell_apply_dirichlet": (_S, [_PI, _PB, _PD, _PD, _PD, _I, _I, _I, _PV]),
    "diffhe_ell_spmv_shared": (_S, [_PD, _PI, _PD, _PD, _I, _PD, _PB, _PD, _I, _I, _I, _PV]),
    "diffhe_cg_workspace_doubles": (_L, [_I, _I]),
    "diffhe_ell_cg_solve": (_S, [_PD, _PI, _PD, _PD, _I, _I, _I, _I, _D, _I, _I, _PD, _PD, _PI, _PI, _PV]),
    "diffhe_ell_galerkin": (_S, [_PD, _PI, _PI, _PD, _PD, _I, _I, _I, _PV]),
    "diffhe_ell_amg_workspace_doubles": (_L, [_AV, _I, _I]),
    "diffhe_ell_amg_pcg_solve": (_S, [_AV, _I, _I, _PD, _PD, _I, _D, _I, _I, _I, _D, _I, _PD, _PD, _PI, _PI, _PV]),
    "diffhe_ell_apply": (_S, [_PD, _PI, _PD, _PD, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_lattice_pcg_workspace_doubles": (_L, [_LV, _I, _I]),
    "diffhe_lattice_pcg_solve": (_S, [_LV, _I, _I, _PD, _PD, _PD, _I, _D, _D, _I, _I, _I, C.POINTER(_D), _I, _PD, _PD,
                                      _PD, _PI, _PI, _PI, _PV]),
    "diffhe_lattice_pcg_profile": (_I, [_I, C.POINTER(_D), C.POINTER(_L)]),
    "diffhe_lattice_kernel_profile": (_I, [_I, C.POINTER(_D), C.POINTER(_L)]),
    "diffhe_lattice_blocks": (_I, [_I, _I]),
    "diffhe_lattice_fused_passes": (_I, []),
    "diffhe_lattice_recompute_ap": (_I, []),
    "diffhe_lattice_apply": (_S, [_LV, _I, _PD, _PD, _PD, _PD, _I, _PV]),
    "diffhe_lattice_smooth": (_S, [_LV, _I, _PD, _PD, _PD, _PD, _D, _I, _PV]),
    "diffhe_lattice_cg_step": (_S, [_LV, _I, _PD, _PV, _I, _PV, _PV, _PD, _PD, _PD, _I, _PD, _PD, _I, _PV]),
    "diffhe_lattice_bilinear": (_I, [_LV, _I, _PD, _PD, _PD, _PD, _PD, _PD, _I, _PV]),
    "diffhe_lattice_apply_shared": (_S, [_I, _I, _I, _PD, _PD, _PD, _I, _PD, _PB, _PD, _I, _PV]),
    "diffhe_lattice_grad_kappa": (_S, [_I, _I, _PD, _I, _PD, _PD, _PD, _PD, _I, _PV]),
    "diffhe_lattice_pack_h16": (_S, [_LV, _I, _PD, _PF, _PV, _PI, _PV]),
    "diffhe_lattice_max_diag": (_S, [_LV, _I, _PD, _PV]),
    "diffhe_lattice_restrict_kappa": (_S, [_PD, _PD, _I, _I, _I, _I, _I, _PV]),
    "diffhe_grad_kappa_blocks": (_I, [_I, _I]),
    "diffhe_p1_grad_kappa": (_S, [_PI, _PD, _PD, _PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_p1_grad_kappa_shared": (_S, [_PI, _PD, _PD, _PD, _PD, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_aniso_gradient_table": (_S, [_PD, _PI, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_aniso_assemble_rows": (_S, [_PD, _PD, _I, _PD, _L, _L, _L, _PI, _PI, _PI, _PB, _PD, _PD, _PD, _I, _I, _I,
                                        _I, _PV]),
    "diffhe_aniso_grad": (_S, [_PI, _PD, _PD, _I, _PD, _PD, _PD, _I, _I, _I, _PD, _L, _L, _PD, _PD, _PV]),
    "diffhe_aniso_grad_shared": (_S, [_PI, _PD, _PD, _I, _PD, _PD, _PD, _I, _I, _I, _I, _PD, _L, _L, _PV]),
    "diffhe_p1_shape_grad": (_S, [_PD, _PI, _I, _I, _I, _I, _PD, _PD, _PD, _L, _L, _PD, _L, _L, _PD, _L, _L, _D, _PI,
                                  _PI, _PD, _PD, _PV]),
    "diffhe_bc_lift": (_S, [_PI, _I, _I, _PD, _PD, _L, _L, _PI, _PD, _L, _L, _PI, _PI, _PI, _I, _PD, _L, _L, _I, _PV]),
    "diffhe_bc_grad": (_S, [_PI, _I, _I, _PD, _PD, _L, _L, _PI, _PI, _PI, _PI, _I, _PD, _L, _L, _PD, _L, _L, _PD, _L,
                            _L, _PD, _L, _L, _PD, _I, _PV]),
    "diffhe_bc_scatter": (_S, [_PI, _I, _PD, _L, _L, _PD, _L, _L, _I, _PV]),
    "diffhe_bc_grad_kappa": (_S, [_PI, _I, _I, _PD, _PI, _PI, _I, _PD, _L, _L, _PD, _L, _L, _PD, _L, _L, _I, _I, _PV]),
    "diffhe_robin_facet_table": (_S, [_PD, _PI, _I, _I, _I, _PD, _PV]),
    "diffhe_robin_assemble": (_S, [_PI, _I, _I, _PD, _PI, _PI, _PI, _PI, _I, _PD, _PD, _L, _L, _PD, _L, _L, _PD, _L, _L,
                                   _PD, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_robin_grad": (_S, [_PI, _I, _I, _PD, _PD, _PD, _PD, _I, _I, _PD, _L, _L, _PD, _L, _L, _PD, _L, _L, _PD, _L,
                               _L, _PD, _L, _L, _PV]),
    "diffhe_robin_sum_blocks": (_I, [_I]),
    "diffhe_robin_sum_facets": (_S, [_PD, _I, _I, _PD, _PD, _PV]),
    "diffhe_ell_sample_scales": (_S, [_PD, _PB, _I, _I, _PD, _PD, _PV]),
    "diffhe_ell_mean_operator": (_S, [_PD, _PD, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_ell_strength_filter": (_S, [_PD, _PI, _I, _I, _D, _PI, _PD, _PV]),
    "diffhe_eig_gram_blocks": (_I, [_I, _I]),
    "diffhe_eig_gram": (_S, [_PD, _PD, _PD, _PB, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_eig_ritz": (_S, [_PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PI, _PV]),
    "diffhe_eig_rotate": (_S, [_PD, _PD, _PD, _PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PD, _PV]),
    "diffhe_eig_residual": (_S, [_PD, _PD, _PD, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_eig_fix_sign": (_S, [_PD, _PD, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_to_node_major": (_S, [_PD, _L, _PB, _PD, _I, _I, _I, _PV]),
    "diffhe_to_sample_major": (_S, [_PD, _PD, _PD, _L, _I, _I, _I, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_elastic.h, the library's second header (linear
# elasticity, csrc/elastic.hip): bound by the same loop of `lib()`, with the same pointer classes and status marker
# (tests/test_elasticity.py holds this table against that header)
ELASTIC_SIGNATURES = {
    "diffhe_elast_assemble_rows": (_S, [_PD, _PD, _I, _D, _D, _PD, _L, _L, _PI, _PI, _PI, _PB, _PD, _PD, _PD, _I, _I,
                                        _I, _I, _PV]),
    "diffhe_elast_grad": (_S, [_PI, _PD, _PD, _I, _D, _D, _PD, _PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_elast_grad_shared": (_S, [_PI, _PD, _PD, _I, _D, _D, _PD, _PD, _PD, _I, _I, _I, _I, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_stress.h, the library's third header (stress recovery of
# elastic solves, csrc/stress.hip): bound by the same loop (tests/test_stress.py holds this table against that header)
STRESS_SIGNATURES = {
    "diffhe_stress_eval": (_S, [_PI, _PD, _I, _D, _D, _D, _PD, _PD, _L, _L, _I, _I, _I, _PD, _L, _L, _PD, _PV]),
    "diffhe_stress_adjoint": (_S, [_PI, _PD, _I, _D, _D, _D, _PD, _PD, _L, _L, _PD, _L, _L, _PD, _PI, _PI, _I, _I, _I, _I,
                                   _PD, _PD, _PD, _PD, _PD, _PV]),
    "diffhe_stress_adjoint_shared": (_S, [_PI, _PD, _I, _D, _D, _D, _PD, _PD, _L, _L, _PD, _L, _L, _PD, _I, _I, _I, _I,
                                          _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_eigenstrain.h, the library's fourth header (eigenstrain
# loads, csrc/eigenstrain.hip, and the eigen variants of the stress entries, csrc/stress.hip): bound by the same loop
# (tests/test_eigenstrain.py holds this table against that header)
_EIGEN_HEAD = [_D, _D, _I, _PD, _L, _L, _PD, _L, _L, _L]    # lam1, mu1, plane_strain, E and its strides, eps0 and its strides
EIGENSTRAIN_SIGNATURES = {
    "diffhe_eigenstrain_load": (_S, [_PI, _PI, _PD, _PD, _I, *_EIGEN_HEAD, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_eigenstrain_load_adjoint": (_S, [_PI, _PD, _PD, _I, *_EIGEN_HEAD, _PD, _I, _I, _I, _I, _PD, _L, _L, _PD, _PD,
                                             _PD, _PV]),
    "diffhe_eigenstrain_load_adjoint_shared": (_S, [_PI, _PD, _PD, _I, *_EIGEN_HEAD, _PD, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_stress_eval_eigen": (_S, [_PI, _PD, _I, _D, _D, _I, _PD, _PD, _L, _L, _PD, _L, _L, _L, _I, _I, _I, _PD, _L, _L,
                                      _PD, _PV]),
    "diffhe_stress_adjoint_eigen": (_S, [_PI, _PD, _I, _D, _D, _I, _PD, _PD, _L, _L, _PD, _L, _L, _L, _PD, _L, _L, _PD, _PI,
                                         _PI, _I, _I, _I, _I, _PD, _PD, _PD, _PD, _PD, _PD, _L, _L, _PV]),
    "diffhe_stress_adjoint_eigen_shared": (_S, [_PI, _PD, _I, _D, _D, _I, _PD, _PD, _L, _L, _PD, _L, _L, _L, _PD, _L, _L,
                                                _PD, _I, _I, _I, _I, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_modal.h, the library's fifth header (vibration modes of
# elastic bodies: the mass and the density gradient of csrc/modal.hip, the block passes of csrc/eigen.hip under a nodal
# mass per sample): bound by the same loop (tests/test_modal.py holds this table against that header)
_MASS = [_PD, _L, _L, _I]       # mass, its strides per node and per sample, unknowns per node
MODAL_SIGNATURES = {
    "diffhe_modal_mass": (_S, [_PI, _PI, _PD, _I, _PD, _L, _L, _I, _I, _I, _I, _PD, _PV]),
    "diffhe_modal_gram": (_S, [_PD, _PD, *_MASS, _PB, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_modal_rotate": (_S, [_PD, _PD, _PD, _PD, *_MASS, _I, _I, _I, _PD, _PD, _PD, _PD, _PV]),
    "diffhe_modal_residual": (_S, [_PD, _PD, *_MASS, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_modal_fix_sign": (_S, [_PD, *_MASS, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_modal_grad_rho": (_S, [_PI, _PD, _I, _PD, _PD, _I, _I, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_modal_grad_rho_shared": (_S, [_PI, _PD, _I, _PD, _PD, _I, _I, _I, _I, _I, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_elastic_shape.h, the library's sixth header (node-coordinate
# gradients of elastic solves and stress evaluations, csrc/elastic_shape.hip): bound by the same loop
# (tests/test_elastic_shape.py holds this table against that header)
ELASTIC_SHAPE_SIGNATURES = {
    "diffhe_elast_shape_grad": (_S, [_PI, _PD, _PD, _I, _D, _D, _PD, _PD, _PD, _PD, _PD, _L, _L, _I, _I, _I, _I, _PI, _PI,
                                     _PD, _PD, _PV]),
    "diffhe_stress_shape_grad": (_S, [_PI, _PD, _I, _D, _D, _D, _PD, _PD, _L, _L, _PD, _L, _L, _PD, _I, _I, _I, _I, _PI,
                                      _PI, _PD, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_elastic_aniso.h, the library's seventh header (elasticity
# with a stiffness tensor per element, csrc/elastic_aniso.hip, and the row bound of lambda_max(D^-1 A) its solver takes for
# the smoother of every level): bound by the same loop (tests/test_elastic_aniso.py holds this table against that header)
ELASTIC_ANISO_SIGNATURES = {
    "diffhe_elastc_assemble_rows": (_S, [_PD, _PD, _I, _PD, _L, _L, _L, _PI, _PI, _PI, _PB, _PD, _PD, _PD, _I, _I, _I,
                                         _I, _PV]),
    "diffhe_elastc_grad": (_S, [_PI, _PD, _PD, _I, _PD, _PD, _PD, _I, _I, _I, _PD, _L, _L, _PD, _PD, _PV]),
    "diffhe_elastc_grad_shared": (_S, [_PI, _PD, _PD, _I, _PD, _PD, _PD, _I, _I, _I, _I, _PD, _L, _L, _PV]),
    "diffhe_ell_jacobi_row_bound": (_S, [_PD, _PI, _I, _I, _I, _PD, _PD, _PV]),
}
ROW_BOUND_BLOCKS = 1024     # DIFFHE_ROW_BOUND_BLOCKS

# name -> (restype, argtypes) of every symbol of include/diffhe_elastic_facets.h, the library's eighth header (tractions,
# pressure and elastic foundations on boundary facets of elastic bodies, csrc/elastic_facets.hip): bound by the same loop
# (tests/test_elastic_facets.py holds this table against that header)
_FACETS = [_PI, _I, _I, _PD, _PD]       # fac, d, nF, area, normal
ELASTIC_FACET_SIGNATURES = {
    "diffhe_elastf_facet_table": (_S, [_PD, _PI, _PI, _I, _I, _I, _PD, _PD, _PV]),
    "diffhe_elastf_assemble": (_S, [*_FACETS, _PI, _PI, _PI, _PI, _I, _PB, _PD, _PD, _L, _L, _L, _PD, _L, _L, _PD, _L, _L,
                                    _PD, _L, _L, _PD, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_elastf_grad": (_S, [*_FACETS, _PD, _PD, _PD, _I, _I, _PD, _L, _L, _L, _PD, _L, _L, _PD, _L, _L, _PD, _L, _L,
                                _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_filter.h, the library's ninth header (the density filter
# on the elements of a P1 mesh and its adjoint, csrc/filter.hip): bound by the same loop (tests/test_density_filter.py
# holds this table against that header)
_CELLS = [_PI, _PI, _PI, _I, _I, _I, _D]       # cell_of, order, cell_start, ncx, ncy, ncz, R
FILTER_SIGNATURES = {
    "diffhe_filter_count": (_S, [_PD, _I, _I, *_CELLS, _PI, _PV]),
    "diffhe_filter_fill": (_S, [_PD, _PD, _I, _I, *_CELLS, _I, _PL, _PI, _PD, _PD, _PV]),
    "diffhe_filter_apply": (_S, [_PD, _PD, _I, _I, _PL, _PI, _PD, _D, _I, _I, _PD, _L, _L, _PD, _L, _L, _I, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_sample.h, the library's tenth header (nodal fields sampled
# at arbitrary points of a P1 mesh and the transpose, csrc/sample.hip): bound by the same loop
# (tests/test_point_sampling.py holds this table against that header)
SAMPLE_SIGNATURES = {
    "diffhe_sample_locate": (_S, [_PD, _PI, _I, _I, _I, _PI, _PI, _I, _I, _I, _PD, _PI, _PI, _I, _D, _PI, _PD, _PD, _PI,
                                  _PV]),
    "diffhe_sample_apply": (_S, [_PI, _I, _I, _PI, _PD, _I, _I, _PD, _L, _L, _L, _PD, _L, _L, _L, _L, _I, _I, _PV]),
    "diffhe_sample_adjoint": (_S, [_PL, _PI, _PI, _I, _I, _I, _PD, _I, _I, _PD, _L, _L, _L, _L, _PD, _L, _L, _L, _I, _I,
                                   _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_hyperelastic.h, the library's eleventh header (finite-strain
# Neo-Hookean elasticity: tangent, internal force, energy and dL/dE, csrc/hyperelastic.hip): bound by the same loop
# (tests/test_hyperelastic.py holds this table against that header)
_HYPER_HEAD = [_PI, _PD, _PD, _I, _D, _D]       # elems, gtab, vol, dim, lam1, mu1
HYPERELASTIC_SIGNATURES = {
    "diffhe_hyper_assemble_rows": (_S, [*_HYPER_HEAD, _PD, _L, _L, _PD, _PI, _PI, _PI, _PB, _PD, _I, _I, _I, _I, _PV]),
    "diffhe_hyper_residual": (_S, [_PI, _PI, *_HYPER_HEAD, _PD, _L, _L, _PD, _I, _I, _I, _PD, _PV]),
    "diffhe_hyper_energy": (_S, [*_HYPER_HEAD, _PD, _L, _L, _PD, _I, _I, _I, _PD, _PD, _PD, _PD, _PV]),
    "diffhe_hyper_grad": (_S, [*_HYPER_HEAD, _PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_hyper_grad_shared": (_S, [*_HYPER_HEAD, _PD, _PD, _I, _I, _I, _I, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_hyper_stress.h, the library's twelfth header (Cauchy stress,
# von Mises stress and energy density of finite-strain solves with their adjoint, csrc/hyper_stress.hip): bound by the same
# loop (tests/test_hyper_stress.py holds this table against that header)
_CAUCHY_HEAD = [_PI, _PD, _I, _D, _D, _PD, _PD, _L, _L]     # elems, gtab, dim, lam1, mu1, u, E and its strides
_CAUCHY_BARS = [_PD, _L, _L, _PD, _PD]                       # sigma_bar, osc, ose, vm_bar, w_bar
HYPER_STRESS_SIGNATURES = {
    "diffhe_hyper_stress_eval": (_S, [*_CAUCHY_HEAD, _I, _I, _I, _PD, _L, _L, _PD, _PD, _PV]),
    "diffhe_hyper_stress_adjoint": (_S, [*_CAUCHY_HEAD, *_CAUCHY_BARS, _PI, _PI, _I, _I, _I, _I, _PD, _PD, _PD, _PD, _PD,
                                         _PV]),
    "diffhe_hyper_stress_adjoint_shared": (_S, [*_CAUCHY_HEAD, *_CAUCHY_BARS, _I, _I, _I, _I, _PD, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_elastic_aniso_stress.h, the library's thirteenth header
# (stress and quadratic failure index of anisotropic elastic solves with their adjoint, csrc/elastic_aniso_stress.hip): bound
# by the same loop (tests/test_elastic_aniso_stress.py holds this table against that header)
_ASTRESS_HEAD = [_PI, _PD, _I, _PD, _PD, _L, _L, _L, _PD, _L, _L, _L]   # elems, gtab, dim, u, C and the criterion with 3 strides each
_ASTRESS_BARS = [_PD, _L, _L, _PD]                                       # sigma_bar, osc, ose, phi_bar
_ASTRESS_GRAD = [_PD, _L, _L, _PD, _PD]                                  # per element and sample with 2 strides, partials, sums
ELASTIC_ANISO_STRESS_SIGNATURES = {
    "diffhe_elastc_stress_eval": (_S, [*_ASTRESS_HEAD, _I, _I, _I, _PD, _L, _L, _PD, _PV]),
    "diffhe_elastc_stress_adjoint": (_S, [*_ASTRESS_HEAD, *_ASTRESS_BARS, _PI, _PI, _I, _I, _I, _I, _PD, _PD,
                                          *_ASTRESS_GRAD, *_ASTRESS_GRAD, _PV]),
    "diffhe_elastc_stress_adjoint_shared": (_S, [*_ASTRESS_HEAD, *_ASTRESS_BARS, _I, _I, _I, _I, _PD, _L, _L, _PD, _L, _L,
                                                 _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_buckling.h, the library's fourteenth header (linear buckling
# of elastic bodies: the geometric stiffness applied from the node pattern, the block passes of a pencil whose right-hand
# matrix is a block, and the cotangent of the prestress, csrc/buckling.hip): bound by the same loop
# (tests/test_buckling.py holds this table against that header)
_MODES = [_PI, _PD, _PD, _I, _PD, _PD, _I, _I, _I, _I, _I]      # elems, gtab, vol, dim, X, w, k, n, m, B, Bp
BUCKLING_SIGNATURES = {
    "diffhe_buckling_apply": (_S, [_PD, _PI, _PB, _PD, _PD, _D, _I, _I, _I, _I, _I, _PV]),
    "diffhe_buckling_step": (_S, [_PD, _PD, _PD, _PD, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_buckling_gram": (_S, [_PD, _PD, _PD, _PB, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_buckling_rotate": (_S, [_PD, _PD, _PD, _PD, _PD, _I, _I, _I, _PD, _PD, _PD, _PD, _PV]),
    "diffhe_buckling_grad_sigma": (_S, [*_MODES, _PD, _L, _L, _PD, _PD, _PV]),
    "diffhe_buckling_grad_sigma_shared": (_S, [*_MODES, _PD, _L, _L, _PV]),
}

# name -> (restype, argtypes) of every symbol of include/diffhe_lobpcg.h, the library's fifteenth header (the block passes of
# the LOBPCG outer iteration on the basis [X | W | P]: Gram matrices, the Ritz step with its fallback, the rotation,
# csrc/lobpcg.hip): bound by the same loop (tests/test_lobpcg.py holds this table against that header)
LOBPCG_SIGNATURES = {
    "diffhe_lobpcg_gram_blocks": (_I, [_I, _I]),
    "diffhe_lobpcg_gram": (_S, [_PD, _PD, _PD, _PB, _I, _I, _I, _PD, _PD, _PD, _PV]),
    "diffhe_lobpcg_ritz": (_S, [_PD, _PD, _I, _I, _I, _I, _PD, _PD, _PI, _PI, _PV]),
    "diffhe_lobpcg_rotate": (_S, [_PD, _PD, _PD, _PD, _PD, _I, _I, _I, _I, _PD, _PD, _PD, _PD, _PV]),
}

_lib = None


class HipExtensionError(RuntimeError):
    pass


CHAIN_REFERENCE_ORDER = 1   # DIFFHE_CHAIN_REFERENCE_ORDER
ELL_SCALE_CHUNK = 256       # DIFFHE_ELL_SCALE_CHUNK
# option bits of the `flags` word of diffhe_lattice_pcg_solve / diffhe_ell_amg_pcg_solve (DIFFHE_PCG_* in diffhe_hip.h)
PCG_FP32 = 1
PCG_FMG = 2
PCG_FMG_CYCLES_SHIFT = 2    # two bits
PCG_NO_FLOOR = 16
PCG_WARM = 32
PCG_UNFUSED = 64
PCG_DENSE_SCALAR = 128
PCG_CLOSED_FP32_STEP = 256
PCG_PRE2 = 512
PCG_RESID_FP64 = 1 << 10   # DIFFHE_PCG_RESID_FP64
PCG_RESID_KEEP_LO = 1 << 11   # DIFFHE_PCG_RESID_KEEP_LO
PCG_TRUST_ITS_SHIFT = 12    # DIFFHE_PCG_TRUST_ITS_SHIFT: four bits
PCG_SPLIT_START = 1 << 16   # DIFFHE_PCG_SPLIT_START


def lib():
    """Load (once) and return the bound library; raise loudly if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipExtensionError(
                f"libdiffhe_hip.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in (*SIGNATURES.items(), *ELASTIC_SIGNATURES.items(), *STRESS_SIGNATURES.items(),
                                  *EIGENSTRAIN_SIGNATURES.items(), *MODAL_SIGNATURES.items(),
                                  *ELASTIC_SHAPE_SIGNATURES.items(), *ELASTIC_ANISO_SIGNATURES.items(),
                                  *ELASTIC_FACET_SIGNATURES.items(), *FILTER_SIGNATURES.items(),
                                  *SAMPLE_SIGNATURES.items(), *HYPERELASTIC_SIGNATURES.items(),
                                  *HYPER_STRESS_SIGNATURES.items(), *ELASTIC_ANISO_STRESS_SIGNATURES.items(),
                                  *BUCKLING_SIGNATURES.items(), *LOBPCG_SIGNATURES.items()):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = (_I if res is _S else res), args
            if res is _S:
                fn.errcheck = _errcheck
        if handle.diffhe_abi_version() != ABI_VERSION:
            raise HipExtensionError("libdiffhe_hip.so ABI version mismatch")
        _lib = handle
    return _lib


def _errcheck(status, func, args):
    """ctypes errcheck of every status entry: a failed call raises under the entry's own name."""
    if status != 0:
        check(status, func.__name__)
    return status


def check(status: int, what: str) -> None:
    if status != 0:
        L = lib()
        msg = L.diffhe_status_string(status).decode()
        if status == -2:
            msg += ": " + L.diffhe_last_hip_error().decode()
        raise HipExtensionError(f"{what} failed: {msg}")


def ptr(t):
    """Device (or pinned host) address of a tensor, or NULL for None."""
    return None if t is None else C.c_void_p(t.data_ptr())
