"""ctypes binding of the C ABI in include/avs.h (libavs_hip.so, built in-tree for gfx950).

This is plumbing only: it declares the prototypes, turns avs_status into exceptions and offers
small helpers to hand torch / numpy buffers across the boundary.  It fails loudly when the HIP
library is missing -- there is no CPU fallback of any kind in the product path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AVS_LIB_PATH", os.path.join(_HERE, "libavs_hip.so"))
PROBE_LIB_PATH = os.environ.get("AVS_PROBE_LIB_PATH", os.path.join(_HERE, "libavs_probe.so"))

MAX_LEVELS = 8
EDGE_STENCIL_CAP, CENTER_STENCIL_CAP = 32, 8
EDGE_BOUNDARY_CAP, CENTER_BOUNDARY_CAP = 4, 2
UNIQUE_ID_BYTES = 128
DIST_BLOB_BYTES = 512

OK, EINVAL, ENOMEM, EHIP, ERCCL, EINTERNAL, ESTATE = range(7)
STATUS_NAMES = {0: "AVS_OK", 1: "AVS_EINVAL", 2: "AVS_ENOMEM", 3: "AVS_EHIP", 4: "AVS_ERCCL",
                5: "AVS_EINTERNAL", 6: "AVS_ESTATE"}
MEM_HOST, MEM_DEVICE = 0, 1
PRECISION_F64, PRECISION_F32 = 0, 1   # avs_desc.precision (SolveType of the reference, util.h:25-37)
(OPTION_PRECONDITIONER, OPTION_RESIDENT_LOOP, OPTION_TRANSPORT, OPTION_PARANOID, OPTION_GRAPH_REPLAY, OPTION_BRICK_FORM,
 OPTION_FUSED_SCALAR_STEPS, OPTION_RELOAD_ENVIRONMENT, OPTION_F32_VECTORS, OPTION_FUSED_VECTOR_UPDATE,
 OPTION_DIST_F32_VECTORS) = range(11)  # avs_set_solver_option
OPTION_RESIDENT_F32 = 12   # (11 is not assigned)
OPTION_RESIDENT_LOCAL_TABLES = 13
OPTION_MIXED_PRECISION = 14
OPTION_DIST_MIXED_PRECISION = 15
USE_TRANSPORT_AUTO, USE_TRANSPORT_RCCL, USE_TRANSPORT_DIRECT = 0, 1, 2
BRICK_AUTO, BRICK_NEVER, BRICK_ALWAYS, BRICK_TUNE = -1, 0, 1, 2
PRECONDITIONER_JACOBI, PRECONDITIONER_NONE = 0, 1
INACTIVE, ACTIVE, UP, DOWN = 0, 1, 2, 3
UNASSIGNED, SOLIDBOUNDARY, OUTSIDE = -1, -2, -3
INDEX_VELOCITY, INDEX_EDGE, INDEX_CENTER = 0, 1, 2
CHECK_LABELS, CHECK_VELOCITY_INDICES = 1, 2   # bits of `what` of avs_check_octree
(RULE_LABEL_VALUE, RULE_COLUMN, RULE_UP, RULE_ACTIVE, RULE_INDEX_VALUE, RULE_FACE, RULE_SENTINEL, RULE_NUMBERING) = range(8)
OCTREE_RULES = 8
CHECK_EDGE_INDICES, CHECK_CENTER_INDICES = 1, 2   # bits of `what` of avs_check_stress_indices
(STRESS_RULE_EDGE_VALUE, STRESS_RULE_EDGE_CELLS, STRESS_RULE_EDGE_FACES, STRESS_RULE_EDGE_NUMBERING, STRESS_RULE_CENTER_VALUE,
 STRESS_RULE_CENTER_LABEL, STRESS_RULE_CENTER_FACES, STRESS_RULE_CENTER_EDGES, STRESS_RULE_CENTER_NUMBERING) = range(9)
STRESS_RULES = 9
RATES_OF_SOLUTION, RATES_OF_INITIAL_GUESS = 0, 1   # `which` of avs_get_strain_rates / avs_get_shear_rate_field
EDGE_LOOKUP_OWN, EDGE_LOOKUP_CHILD, EDGE_LOOKUP_GRANDCHILD, EDGE_LOOKUP_SKIPPED = range(4)   # avs_strain_summary.edge_lookups
VISCOSITY_CARREAU_YASUDA, VISCOSITY_HERSCHEL_BULKLEY = 0, 1   # avs_viscosity_model.kind
CHECK_OF_SOLUTION, CHECK_OF_INITIAL_GUESS = 0, 1   # `which` of avs_check_solution
SPECTRUM_OF_JACOBI, SPECTRUM_OF_MATRIX = 0, 1   # `op` of avs_estimate_spectrum
SPECTRUM_START_RESIDUAL, SPECTRUM_START_HASH, SPECTRUM_START_VECTOR = 0, 1, 2   # its `start`
SPECTRUM_MAX_STEPS = 512
PREPASS_OPTION_FINE_BANDWIDTH = 0   # avs_prepass_set_option
PREPASS_OPTION_APPLY_SOLID_WEIGHTS = 1   # ... the reference's "Apply Solid Weights": 0 off (default), 1 on
REFINEMENT_MAX_DILATE = 16          # avs_prepass_set_refinement: dilate_cells in 0 .. 16
CSR_CHECK_VALUES, CSR_CHECK_ORDER, CSR_CHECK_DIAGONAL, CSR_CHECK_SYMMETRY, CSR_CHECK_ALL = 1, 2, 4, 8, 15   # bits of `what` of avs_check_csr
(CSR_RULE_ROW_PTR, CSR_RULE_COLUMN, CSR_RULE_VALUE, CSR_RULE_VECTOR, CSR_RULE_ORDER, CSR_RULE_DIAGONAL, CSR_RULE_PATTERN,
 CSR_RULE_SYMMETRY) = range(8)
CSR_RULES = 8
(FIELD_CENTER_WEIGHTS, FIELD_EDGE_WEIGHTS, FIELD_FACE_WEIGHTS, FIELD_VISCOSITY, FIELD_DENSITY,
 FIELD_VELOCITY, FIELD_SOLID_VELOCITY) = range(7)

# every symbol include/avs.h declares (checked by tests/test_capi_symbols.py)
EXPORTED_SYMBOLS = [
    "avs_last_error", "avs_version", "avs_abi_version", "avs_cancel", "avs_cancel_clear", "avs_create", "avs_destroy", "avs_set_labels",
    "avs_set_index_field", "avs_set_dof_counts", "avs_set_scalar_field", "avs_build_stencils",
    "avs_build_initial_guess", "avs_build_system", "avs_assemble", "avs_solve", "avs_set_solver_option",
    "avs_get_assembly_info", "avs_get_matrix_format", "avs_get_solution", "avs_get_initial_guess", "avs_get_csr",
    "avs_get_edge_stencils", "avs_get_center_stencils", "avs_pcg_csr",
    "avs_prepass_create", "avs_prepass_destroy", "avs_prepass_run",
    "avs_prepass_get_info", "avs_prepass_get_labels", "avs_prepass_get_mask", "avs_prepass_get_index",
    "avs_prepass_get_weights", "avs_prepass_get_regular_index", "avs_prepass_apply", "avs_set_regular_index_field",
    "avs_transfer_to_regular_grid", "avs_transfer_to_regular_grid_in_place", "avs_get_node_grid", "avs_get_dof_table", "avs_plan_owners", "avs_plan_create", "avs_plan_get_sizes",
    "avs_plan_get_arrays", "avs_plan_destroy", "avs_dist_get_unique_id", "avs_dist_init",
    "avs_local_group_create", "avs_local_group_destroy", "avs_dist_init_local", "avs_dist_partition",
    "avs_spmv_tile_rows", "avs_dist_assemble", "avs_dist_get_plan_sizes", "avs_dist_get_overlap_tiles", "avs_dist_get_plan_arrays", "avs_dist_solve", "avs_dist_get_solution",
    "avs_dist_get_info", "avs_dist_init_hosted", "avs_dist_export_blob", "avs_dist_import_blobs",
    "avs_prepass_set_slab", "avs_prepass_get_window", "avs_dist_bind_prepass", "avs_dist_get_cuts", "avs_set_solution",
    "avs_sample_velocity", "avs_get_octree_cells", "avs_prepass_get_octree_cells", "avs_check_octree", "avs_prepass_check_octree",
    "avs_check_csr", "avs_check_system", "avs_check_stress_indices", "avs_prepass_check_stress_indices",
    "avs_get_strain_rates", "avs_get_shear_rate_field", "avs_apply_viscosity_model", "avs_check_solution", "avs_check_csr_solution",
    "avs_estimate_spectrum", "avs_estimate_csr_spectrum",
    "avs_prepass_set_option", "avs_prepass_set_refinement", "avs_prepass_get_refinement", "avs_prepass_get_refinement_info",
    "avs_prepass_get_solid_weights_info",
]
# avs_allreduce_i32_fn: avs_status (*)(int32_t *device_data, int64_t count, void *stream, void *user)
ALLREDUCE_I32_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
# include/avs_probe.h: exported by libavs_probe.so only (the -DAVS_PROBES build of the same sources)
PROBE_SYMBOLS = ["avs_spmv_csr", "avs_bench_spmv", "avs_spmv_sell", "avs_bench_stream", "avs_brick_spmv_probe", "avs_spmv_solver_form",
                 "avs_dist_spmv_local_form", "avs_brick_wave_stats", "avs_spmv_csr_form", "avs_vector_update_probe", "avs_pcg_csr_plan",
                 "avs_merge_triplets_probe", "avs_exclusive_scan_probe", "avs_resident_plan_host", "avs_brick_form_probe", "avs_pcg_scalar_probe",
                 "avs_sr_vector_probe", "avs_dist_plan_probe", "avs_phase_loop_info", "avs_viscosity_lattice_probe",
                 "avs_prepass_plan_host"]
DIST_PLAN_PROBE_PLAN, DIST_PLAN_PROBE_TAIL = 0, 1   # avs_dist_plan_probe modes
BRICK_PROBE_FUSED_DOT, BRICK_PROBE_F32, BRICK_PROBE_MIXED, BRICK_PROBE_VALUE_CODES, BRICK_PROBE_DONE = 1, 2, 4, 8, 16   # avs_brick_form_probe flags
VECTOR_PROBE_F32, VECTOR_PROBE_DS, VECTOR_PROBE_CODED, VECTOR_PROBE_KEEP, VECTOR_PROBE_FUSED = 1, 2, 4, 8, 16   # avs_vector_update_probe flags
VECTOR_PROBE_ONE_LAUNCH = 32                                                                                   # ... k_update_fused instead of the pair
(SCALAR_PROBE_REDUCE_LAUNCH, SCALAR_PROBE_REDUCE, SCALAR_PROBE_REDUCE_MB, SCALAR_PROBE_REDUCE_PAIR, SCALAR_PROBE_SCALAR,
 SCALAR_PROBE_MIXED_FINISH_INIT, SCALAR_PROBE_MIXED_FINISH, SCALAR_PROBE_SR_MIXED_BEGIN, SCALAR_PROBE_SR_MIXED_STEP) = range(9)   # avs_pcg_scalar_probe
SCALAR_PROBE_STAGE_NAN = 0x7ff8a5a500000000
SR_PROBE_INIT, SR_PROBE_UPDATE, SR_PROBE_MIXED_RESIDUAL, SR_PROBE_MIXED_RESIDUAL_INIT = range(4)   # avs_sr_vector_probe kernels
SPMV_FORM_FUSED_DOT, SPMV_FORM_F32, SPMV_FORM_NO_CACHE_HINT = 1, 2, 4   # avs_spmv_csr_form flags (include/avs_probe.h)
_VOID_RETURN = ("avs_last_error", "avs_version", "avs_destroy", "avs_plan_destroy", "avs_local_group_destroy",
                "avs_prepass_destroy")


class AvsError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class Desc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("dx", C.c_double),
                ("dt", C.c_double), ("levels", C.c_int32), ("use_enhanced_gradients", C.c_int32),
                ("device", C.c_int32), ("stream", C.c_void_p),
                ("field_nx", C.c_int32), ("field_ny", C.c_int32), ("field_nz", C.c_int32), ("precision", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("error", C.c_double),
                ("rhs_norm2", C.c_double), ("n", C.c_int64), ("nnz", C.c_int64),
                ("solve_ms", C.c_double), ("spmv_ms", C.c_double), ("resident", C.c_int32), ("cancelled", C.c_int32)]


class PlanSizes(C.Structure):
    _fields_ = [("n_own", C.c_int64), ("n_halo", C.c_int64), ("nnz_local", C.c_int64), ("n_send", C.c_int64),
                ("n_peers", C.c_int32)]


class PrepassDesc(C.Structure):
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("dx", C.c_double),
                ("desired_levels", C.c_int32), ("n_super", C.c_int32), ("extrapolation_scale", C.c_double),
                ("device", C.c_int32), ("stream", C.c_void_p),
                ("field_nx", C.c_int32), ("field_ny", C.c_int32), ("field_nz", C.c_int32)]


class PrepassInfo(C.Structure):
    _fields_ = [("levels", C.c_int32), ("n_velocity", C.c_int64), ("n_edge", C.c_int64), ("n_center", C.c_int64),
                ("n_regular", C.c_int64), ("weights_ms", C.c_double), ("octree_ms", C.c_double), ("classify_ms", C.c_double),
                ("number_ms", C.c_double)]


class RefinementInfo(C.Structure):
    """avs_refinement_info: what avs_prepass_get_refinement_info reports about the refinement flags"""
    _fields_ = [("struct_size", C.c_int32), ("dilate_cells", C.c_int32), ("threshold", C.c_float), ("active", C.c_int32),
                ("seeds", C.c_int64), ("flagged", C.c_int64), ("refined", C.c_int64), ("set_ms", C.c_double)]


class SolidWeightsInfo(C.Structure):
    """avs_solid_weights_info: what the last run's weights pass did with the solid SDF; [4] = centre, edge x, edge y, edge z"""
    _fields_ = [("struct_size", C.c_int32), ("enabled", C.c_int32), ("applied", C.c_int32), ("extrapolation", C.c_float),
                ("modified", C.c_int64 * 4), ("zeroed", C.c_int64 * 4), ("above_one", C.c_int64 * 4), ("max_weight", C.c_float * 4),
                ("near_bricks", C.c_int64)]


class AssemblyInfo(C.Structure):
    _fields_ = [("n_velocity", C.c_int64), ("n_edge", C.c_int64), ("n_center", C.c_int64),
                ("nnz", C.c_int64), ("raw_triplets", C.c_int64), ("stencil_ms", C.c_double),
                ("guess_ms", C.c_double), ("system_ms", C.c_double), ("csr_ms", C.c_double)]


class DistInfo(C.Structure):
    _fields_ = [("world_size", C.c_int32), ("rccl_ranks", C.c_int32), ("transport", C.c_int32), ("graph_replay", C.c_int32),
                ("launches_per_iteration", C.c_int32), ("collectives_per_iteration", C.c_int32),
                ("selftest_rounds", C.c_int32), ("paranoid", C.c_int32), ("selftest_bad_entries", C.c_int64)]


class MatrixFormat(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reordered", C.c_int32), ("value_table_size", C.c_int32), ("column_bits", C.c_int32),
                ("bytes_per_nonzero", C.c_int32), ("tile_local_tables", C.c_int32),
                ("column_windows", C.c_int32), ("brick_tiles", C.c_int32), ("brick_patterns", C.c_int32), ("_pad", C.c_int32),
                ("brick_pattern_rows", C.c_int64), ("brick_bytes", C.c_int64), ("brick_walk", C.c_int32), ("brick_value_codes", C.c_int32),
                ("fused_vector_update", C.c_int32), ("fused_vector_faults", C.c_int32), ("float_vectors", C.c_int32),
                ("reliable_updates", C.c_int32)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(MatrixFormat)


class OctreeCheck(C.Structure):
    """avs_octree_check: the report of avs_check_octree / avs_prepass_check_octree"""
    _fields_ = [("struct_size", C.c_int32), ("passed", C.c_int32), ("violations", C.c_int64 * OCTREE_RULES), ("first_rule", C.c_int32),
                ("first_level", C.c_int32), ("first_axis", C.c_int32), ("first_ijk", C.c_int32 * 3)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(OctreeCheck)


class StressCheck(C.Structure):
    """avs_stress_check: the report of avs_check_stress_indices / avs_prepass_check_stress_indices"""
    _fields_ = [("struct_size", C.c_int32), ("passed", C.c_int32), ("violations", C.c_int64 * STRESS_RULES), ("first_rule", C.c_int32),
                ("first_level", C.c_int32), ("first_axis", C.c_int32), ("first_ijk", C.c_int32 * 3), ("active_edges", C.c_int64),
                ("active_centers", C.c_int64)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(StressCheck)


class StrainSummary(C.Structure):
    """avs_strain_summary: the counters, dissipations and maxima of avs_get_strain_rates"""
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("n_edge", C.c_int64), ("n_center", C.c_int64),
                ("empty_edges", C.c_int64), ("empty_centers", C.c_int64), ("boundary_edges", C.c_int64), ("boundary_centers", C.c_int64),
                ("nonfinite", C.c_int64), ("edge_lookups", C.c_int64 * 4), ("empty_pairs", C.c_int64),
                ("dissipation_edge", C.c_double), ("dissipation_center", C.c_double), ("max_abs_edge_rate", C.c_double),
                ("max_abs_center_rate", C.c_double), ("max_shear_rate", C.c_double)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(StrainSummary)


class ViscosityModel(C.Structure):
    """avs_viscosity_model: kind (VISCOSITY_*), the parameters of the two kinds, the clamp and the relaxation of avs_apply_viscosity_model"""
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("mu_0", C.c_double), ("mu_inf", C.c_double), ("lambda_", C.c_double),
                ("a", C.c_double), ("n", C.c_double), ("consistency", C.c_double), ("tau_y", C.c_double), ("regularisation", C.c_double),
                ("mu_min", C.c_double), ("mu_max", C.c_double), ("relaxation", C.c_double)]

    def __init__(self, *a, **k):
        k.setdefault("relaxation", 1.0)
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ViscosityModel)


class ViscositySummary(C.Structure):
    """avs_viscosity_summary: the counts and extrema of avs_apply_viscosity_model"""
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("kind", C.c_int32), ("installed", C.c_int32), ("n_center", C.c_int64),
                ("covered", C.c_int64), ("fringe", C.c_int64), ("untouched", C.c_int64), ("clamped_low", C.c_int64),
                ("clamped_high", C.c_int64), ("nonfinite", C.c_int64), ("min_viscosity", C.c_double), ("max_viscosity", C.c_double),
                ("max_shear_rate", C.c_double), ("max_relative_change", C.c_double)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ViscositySummary)


class CsrCheck(C.Structure):
    """avs_csr_check: the report of avs_check_csr / avs_check_system"""
    _fields_ = [("struct_size", C.c_int32), ("passed", C.c_int32), ("evaluated", C.c_int32), ("first_rule", C.c_int32),
                ("first_index", C.c_int64), ("first_row", C.c_int32), ("first_col", C.c_int32), ("violations", C.c_int64 * CSR_RULES),
                ("empty_rows", C.c_int64), ("longest_row", C.c_int64), ("asymmetric_entries", C.c_int64),
                ("max_abs_value", C.c_double), ("max_abs_asymmetry", C.c_double)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(CsrCheck)


class SolutionCheck(C.Structure):
    """avs_solution_check: the report of avs_check_solution / avs_check_csr_solution"""
    _fields_ = [("struct_size", C.c_int32), ("which", C.c_int32), ("evaluated", C.c_int32), ("claimed_converged", C.c_int32),
                ("claimed_iterations", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("nnz", C.c_int64),
                ("nonfinite_x", C.c_int64), ("nonfinite_b", C.c_int64), ("nonfinite_residual", C.c_int64), ("rows_summed", C.c_int64),
                ("rhs_norm2", C.c_double), ("residual_norm2", C.c_double), ("relative_residual", C.c_double),
                ("max_abs_residual", C.c_double), ("max_residual_row", C.c_int64), ("max_abs_x", C.c_double),
                ("x_dot_ax", C.c_double), ("x_dot_b", C.c_double), ("update_norm2", C.c_double), ("max_abs_update", C.c_double),
                ("claimed_error", C.c_double)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(SolutionCheck)


class Spectrum(C.Structure):
    """avs_spectrum: the report of avs_estimate_spectrum / avs_estimate_csr_spectrum"""
    _fields_ = [("struct_size", C.c_int32), ("evaluated", C.c_int32), ("op", C.c_int32), ("start", C.c_int32), ("steps_asked", C.c_int32),
                ("steps_taken", C.c_int32), ("breakdown", C.c_int32), ("nonfinite", C.c_int32), ("indefinite", C.c_int32),
                ("n", C.c_int64), ("nnz", C.c_int64), ("bad_diagonal", C.c_int64), ("start_norm", C.c_double), ("lambda_min", C.c_double),
                ("lambda_max", C.c_double), ("lambda_min_bound", C.c_double), ("lambda_max_bound", C.c_double),
                ("gershgorin_max", C.c_double), ("condition_estimate", C.c_double), ("tolerance", C.c_double),
                ("iteration_bound", C.c_int64)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(Spectrum)


class ResidentPlanInfo(C.Structure):
    """avs_resident_plan_info (include/avs_probe.h): the CU-resident loop's plan of an avs_pcg_csr_plan solve"""
    _fields_ = [("struct_size", C.c_int32), ("used", C.c_int32), ("workgroups", C.c_int32), ("max_lanes_per_workgroup", C.c_int32),
                ("lanes", C.c_int64), ("max_rows_per_workgroup", C.c_int32), ("lc_bits", C.c_int32), ("ng", C.c_int32),
                ("lds_bytes", C.c_int32), ("max_quads", C.c_int32), ("long_row_lanes", C.c_int32), ("longest_tail", C.c_int32),
                ("max_lane_streamed_rows", C.c_int32), ("streamed_rows", C.c_int64), ("streamed_words", C.c_int64),
                ("max_remote", C.c_int32), ("remap_passes", C.c_int32), ("local_tables", C.c_int32),
                ("tables_per_workgroup", C.c_int32), ("largest_table", C.c_int32), ("why", C.c_char * 128)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ResidentPlanInfo)


class PhaseLoopReport(C.Structure):
    """avs_phase_loop_report (include/avs_probe.h): what the launch-per-phase PCG loop did in the calling thread's last solve"""
    _fields_ = [(k, C.c_int32) for k in (
        "struct_size", "solves", "chunks_launched", "chunks_replayed", "graphs_captured", "graph_broken", "alpha_folded", "alpha_launched",
        "coded", "keep", "fuse_beta", "fuse_vectors", "g", "nb", "float_vectors", "reserved")]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PhaseLoopReport)


class ResidentHostPlanInfo(C.Structure):
    """avs_resident_host_plan_info (include/avs_probe.h): what the host-only planner of the CU-resident loop made of a row-pointer array"""
    _fields_ = [("struct_size", C.c_int32), ("refused", C.c_int32), ("lanes", C.c_int64), ("long_row_lanes", C.c_int32),
                ("longest_tail", C.c_int32), ("max_lane_streamed_rows", C.c_int32), ("max_rows_per_workgroup", C.c_int32),
                ("streamed_rows", C.c_int64), ("streamed_words", C.c_int64), ("stream_T", C.c_double), ("why", C.c_char * 128)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(ResidentHostPlanInfo)


class PrepassPlanInfo(C.Structure):
    """avs_prepass_plan_info (include/avs_probe.h): level cap, slab ranges per level and the numbering's tile layout of a pre-pass run"""
    _fields_ = ([("struct_size", C.c_int32), ("levels", C.c_int32)]
                + [(f"{r}_{e}", C.c_int32 * MAX_LEVELS) for r in ("win", "nl", "v", "p1") for e in ("lo", "hi")]
                + [("level_tile0", C.c_int32 * (MAX_LEVELS + 1) * 4), ("tile0_of", C.c_int32 * 3 * MAX_LEVELS * 4),
                   ("seg", C.c_int64 * 5), ("n_exchange", C.c_int64)])

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(PrepassPlanInfo)


class TripletMergeInfo(C.Structure):
    """avs_triplet_merge_info (include/avs_probe.h): the limits of the device triplet merge and what an avs_merge_triplets_probe run reached"""
    _fields_ = [("struct_size", C.c_int32), ("fast_limit", C.c_int32), ("wave_limit", C.c_int32), ("merge_lds", C.c_int32),
                ("scan_tile", C.c_int32), ("long_grid_waves", C.c_int32), ("long_rows", C.c_int32), ("reserved", C.c_int32),
                ("raw_slots", C.c_int64)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(TripletMergeInfo)


class BrickFormInfo(C.Structure):
    """avs_brick_form_info (include/avs_probe.h): the limits of the brick-structured SpMV form and what an avs_brick_form_probe build made"""
    _fields_ = [("struct_size", C.c_int32)] + [(k, C.c_int32) for k in (
        "run_len", "max_runs", "fast_runs", "pat_max", "pat_words", "pat_words_vc", "pat_len", "x_slots", "park_words", "emode_words",
        "emode_words_mixed", "min_rows", "max_rows", "etile_rows", "tile_vals", "table_max", "block_words", "header_words",
        "ready", "vc", "wide", "col_bits", "tiles", "patterns", "halo_tiles", "grid", "max_walk", "planned", "table_size", "reserved")] + [
        ("pattern_rows", C.c_int64), ("streamed_rows", C.c_int64), ("streamed_words", C.c_int64)]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(BrickFormInfo)


class DistPlanInput(C.Structure):
    """avs_dist_plan_input (include/avs_probe.h): the device arrays avs_dist_plan_probe runs a planner core on"""
    _fields_ = [("n", C.c_int64), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("val", C.c_void_p), ("dof", C.c_void_p), ("perm", C.c_void_p),
                ("owner", C.c_void_p), ("dom", C.c_void_p), ("n_dom", C.c_int64), ("levels", C.c_int32), ("cut_axis", C.c_int32),
                ("extent", C.c_int32), ("split", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32)]


class DistPlanOutput(C.Structure):
    """avs_dist_plan_output: host arrays (and their capacities) the probe copies the plan to"""
    _fields_ = [(k, C.c_int64) for k in ("row_capacity", "nnz_capacity", "send_capacity", "plane_capacity")] + [(k, C.c_void_p) for k in (
        "weights", "plane_owner", "owner", "own_global", "halo_global", "row_ptr_local", "col_local", "val_local", "send_idx", "peers",
        "send_counts", "recv_counts", "tiles_int", "tiles_bnd", "local_ref", "rhs_local")]


class DistPlanInfo(C.Structure):
    """avs_dist_plan_info: the limits the device planners were compiled with and the sizes of the plan an avs_dist_plan_probe run made"""
    _fields_ = [("struct_size", C.c_int32)] + [(k, C.c_int32) for k in (
        "lds_planes", "scan_tile", "spmv_tile_rows", "row_group", "max_world", "nplanes", "n_peers", "n_tiles_int", "n_tiles_bnd")] + [
        (k, C.c_int64) for k in ("n_own", "n_halo", "n_send", "nnz_local", "n_interior", "guard_bytes_hit")]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.struct_size = C.sizeof(DistPlanInfo)


def source_fingerprint():
    """sha256 (16 hex digits) over the library's sources: kernels, internal headers, the public header.  Counter records under
    profiles/ carry the fingerprint of the tree they were taken with; bench.py only quotes a record whose fingerprint is the running one."""
    import glob
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(csrc, "*.inl")) +
                   glob.glob(os.path.join(csrc, "*.cpp")) + [os.path.join(csrc, "Makefile")] +
                   glob.glob(os.path.join(os.path.dirname(csrc), "..", "include", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


_lib = None
_probe_lib = None


def load_probe():
    """libavs_probe.so: the product sources built with -DAVS_PROBES (+ the entries of include/avs_probe.h).  Tools and tests only."""
    return load(probe=True)


def load(probe=False):
    """Load libavs_hip.so (or the probe build); raises if it has not been built (python __graft_entry__.py build)."""
    global _lib, _probe_lib
    if probe and _probe_lib is not None:
        return _probe_lib
    if not probe and _lib is not None:
        return _lib
    path = PROBE_LIB_PATH if probe else LIB_PATH
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(path)
    vp, i32, i64, f64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float
    L.avs_last_error.restype = C.c_char_p
    L.avs_version.restype = C.c_char_p
    L.avs_create.argtypes = [C.POINTER(Desc), C.POINTER(vp)]
    L.avs_destroy.argtypes = [vp]
    L.avs_destroy.restype = None
    L.avs_set_labels.argtypes = [vp, i32, vp, i32]
    L.avs_set_index_field.argtypes = [vp, i32, i32, i32, vp, i32]
    L.avs_set_dof_counts.argtypes = [vp, i64, i64, i64]
    L.avs_set_scalar_field.argtypes = [vp, i32, i32, vp, f32, i32]
    L.avs_build_stencils.argtypes = [vp]
    L.avs_build_initial_guess.argtypes = [vp]
    L.avs_build_system.argtypes = [vp]
    L.avs_assemble.argtypes = [vp, C.POINTER(AssemblyInfo)]
    L.avs_solve.argtypes = [vp, f64, i32, C.POINTER(SolveInfo)]
    L.avs_cancel.argtypes = [vp]
    L.avs_cancel_clear.argtypes = [vp]
    L.avs_abi_version.restype = C.c_int32
    L.avs_set_solver_option.argtypes = [vp, i32, i32]
    L.avs_get_assembly_info.argtypes = [vp, C.POINTER(AssemblyInfo)]
    L.avs_get_matrix_format.argtypes = [vp, C.POINTER(MatrixFormat)]
    L.avs_get_solution.argtypes = [vp, vp, i64, i32]
    L.avs_get_initial_guess.argtypes = [vp, vp, i64, i32]
    L.avs_set_solution.argtypes = [vp, vp, i64, i32]
    L.avs_get_csr.argtypes = [vp, vp, vp, vp, vp, i32]
    L.avs_get_edge_stencils.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
    L.avs_get_center_stencils.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
    L.avs_pcg_csr.argtypes = [i64, vp, vp, vp, vp, vp, f64, i32, i32, i32, vp, C.POINTER(SolveInfo)]
    if probe:
        L.avs_spmv_csr.argtypes = [i64, vp, vp, vp, vp, vp, i32, i32, vp]
        L.avs_bench_spmv.argtypes = [vp, i32, i32, C.POINTER(f64)]
        L.avs_spmv_sell.argtypes = [i64, vp, vp, vp, vp, vp, i32, vp, C.POINTER(f64)]
        L.avs_bench_stream.argtypes = [i32, i64, i32, i32, C.POINTER(f64)]
        L.avs_spmv_solver_form.argtypes = [vp, vp, vp, i32, C.POINTER(f64)]
        L.avs_dist_spmv_local_form.argtypes = [vp, vp, vp, i32, C.POINTER(f64)]
        L.avs_brick_wave_stats.argtypes = [vp, C.POINTER(f64)]
        L.avs_spmv_csr_form.argtypes = [i64, vp, vp, vp, vp, vp, i32, C.POINTER(f64), C.POINTER(MatrixFormat), vp]
        L.avs_vector_update_probe.argtypes = [i32, i32, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        L.avs_pcg_scalar_probe.argtypes = [i32, vp, i32, i32, vp, i32, i32, i32, f64, i32, i32, i32, vp, i32, vp, vp, vp]
        L.avs_sr_vector_probe.argtypes = [i32, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
        L.avs_pcg_csr_plan.argtypes = L.avs_pcg_csr.argtypes + [C.POINTER(ResidentPlanInfo)]
        L.avs_merge_triplets_probe.argtypes = [i64, vp, vp, vp, i32, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(TripletMergeInfo), vp]
        L.avs_exclusive_scan_probe.argtypes = [vp, vp, i64, vp]
        L.avs_resident_plan_host.argtypes = [i64, vp, i32, i32, f64, i32, f64, vp, vp, vp, vp, vp, C.POINTER(ResidentHostPlanInfo)]
        L.avs_brick_form_probe.argtypes = [i64, i64, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, i32, i32, i32, C.POINTER(f64), vp, i32,
                                           C.POINTER(BrickFormInfo), vp, i32, vp]
        L.avs_dist_plan_probe.argtypes = [i32, C.POINTER(DistPlanInput), C.POINTER(DistPlanOutput), C.POINTER(DistPlanInfo), vp]
        L.avs_phase_loop_info.argtypes = [C.POINTER(PhaseLoopReport)]
        L.avs_viscosity_lattice_probe.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(i32), i32]
        L.avs_prepass_plan_host.argtypes = [vp, i32, i32, vp, i32, i32, C.POINTER(PrepassPlanInfo)]
    L.avs_prepass_create.argtypes = [C.POINTER(PrepassDesc), C.POINTER(vp)]
    L.avs_prepass_destroy.argtypes = [vp]
    L.avs_prepass_destroy.restype = None
    L.avs_prepass_run.argtypes = [vp, vp, vp, i32]
    L.avs_prepass_get_info.argtypes = [vp, C.POINTER(PrepassInfo)]
    L.avs_prepass_get_labels.argtypes = [vp, i32, vp, i32]
    L.avs_prepass_get_mask.argtypes = [vp, vp, i32]
    L.avs_prepass_get_index.argtypes = [vp, i32, i32, i32, vp, i32]
    L.avs_prepass_get_weights.argtypes = [vp, i32, i32, vp, i32]
    L.avs_prepass_apply.argtypes = [vp, vp]
    L.avs_prepass_get_regular_index.argtypes = [vp, i32, vp, i32]
    L.avs_prepass_set_option.argtypes = [vp, i32, f64]
    L.avs_prepass_set_refinement.argtypes = [vp, vp, f32, i32, i32]
    L.avs_prepass_get_refinement.argtypes = [vp, vp, i32]
    L.avs_prepass_get_refinement_info.argtypes = [vp, C.POINTER(RefinementInfo)]
    L.avs_prepass_get_solid_weights_info.argtypes = [vp, C.POINTER(SolidWeightsInfo)]
    L.avs_set_regular_index_field.argtypes = [vp, i32, vp, i32]
    L.avs_transfer_to_regular_grid.argtypes = [vp, vp, vp, vp, i32]
    L.avs_transfer_to_regular_grid_in_place.argtypes = [vp, vp, vp, vp]
    L.avs_get_node_grid.argtypes = [vp, i32, vp, vp, vp, vp, i32]
    L.avs_sample_velocity.argtypes = [vp, i64, vp, vp, vp, vp, i32]
    L.avs_get_octree_cells.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i32]
    L.avs_prepass_get_octree_cells.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i32]
    L.avs_check_octree.argtypes = [vp, C.c_uint32, C.POINTER(OctreeCheck)]
    L.avs_prepass_check_octree.argtypes = [vp, C.c_uint32, C.POINTER(OctreeCheck)]
    L.avs_check_stress_indices.argtypes = [vp, C.c_uint32, C.POINTER(StressCheck)]
    L.avs_prepass_check_stress_indices.argtypes = [vp, C.c_uint32, C.POINTER(StressCheck)]
    L.avs_get_strain_rates.argtypes = [vp, i32, vp, vp, vp, C.POINTER(StrainSummary), i32]
    L.avs_get_shear_rate_field.argtypes = [vp, i32, vp, i32]
    L.avs_apply_viscosity_model.argtypes = [vp, i32, C.POINTER(ViscosityModel), vp, i32, C.POINTER(ViscositySummary), i32]
    L.avs_check_csr.argtypes = [i64, i64, vp, vp, vp, vp, vp, C.c_uint32, f64, i32, i32, vp, C.POINTER(CsrCheck)]
    L.avs_check_system.argtypes = [vp, C.c_uint32, f64, C.POINTER(CsrCheck)]
    L.avs_check_solution.argtypes = [vp, i32, vp, C.POINTER(SolutionCheck), i32]
    L.avs_check_csr_solution.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(SolutionCheck)]
    L.avs_estimate_spectrum.argtypes = [vp, i32, i32, i32, f64, vp, vp, vp, vp, vp, i32, C.POINTER(Spectrum)]
    L.avs_estimate_csr_spectrum.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, i32, f64, vp, vp, vp, vp, vp, i32, i32, vp,
                                            C.POINTER(Spectrum)]
    L.avs_get_dof_table.argtypes = [vp, i32, vp, i32]
    L.avs_plan_owners.argtypes = [i64, vp, vp, i32, i32, i32, i32, vp]
    L.avs_plan_create.argtypes = [i64, vp, vp, vp, i32, i32, C.POINTER(vp)]
    L.avs_plan_get_sizes.argtypes = [vp, C.POINTER(PlanSizes)]
    L.avs_plan_get_arrays.argtypes = [vp] + [vp] * 9
    L.avs_plan_destroy.argtypes = [vp]
    L.avs_plan_destroy.restype = None
    L.avs_dist_get_unique_id.argtypes = [vp]
    L.avs_dist_init.argtypes = [vp, vp, i32, i32]
    L.avs_local_group_create.argtypes = [i32, C.POINTER(vp)]
    L.avs_local_group_destroy.argtypes = [vp]
    L.avs_local_group_destroy.restype = None
    L.avs_dist_init_local.argtypes = [vp, vp, i32]
    L.avs_dist_partition.argtypes = [vp, i32]
    L.avs_dist_get_plan_sizes.argtypes = [vp, C.POINTER(PlanSizes)]
    L.avs_dist_assemble.argtypes = [vp, i32, C.POINTER(AssemblyInfo)]
    L.avs_spmv_tile_rows.argtypes = []
    L.avs_spmv_tile_rows.restype = i32
    L.avs_dist_get_overlap_tiles.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.avs_dist_get_plan_arrays.argtypes = [vp] + [vp] * 9
    L.avs_dist_solve.argtypes = [vp, f64, i32, C.POINTER(SolveInfo)]
    L.avs_dist_get_solution.argtypes = [vp, vp, i64, i32]
    L.avs_dist_get_info.argtypes = [vp, C.POINTER(DistInfo)]
    L.avs_dist_init_hosted.argtypes = [vp, i32, i32]
    L.avs_dist_export_blob.argtypes = [vp, vp]
    L.avs_dist_import_blobs.argtypes = [vp, vp]
    L.avs_prepass_set_slab.argtypes = [vp, i32, vp, i32, i32, ALLREDUCE_I32_FN, vp]
    L.avs_prepass_get_window.argtypes = [vp, vp, vp, vp]
    L.avs_dist_bind_prepass.argtypes = [vp, vp, i32, vp]
    L.avs_dist_get_cuts.argtypes = [vp, i32, C.POINTER(i32), vp]
    for name in EXPORTED_SYMBOLS + (PROBE_SYMBOLS if probe else []):
        fn = getattr(L, name)
        if name not in _VOID_RETURN:
            fn.restype = C.c_int
    if probe:
        _probe_lib = L
    else:
        _lib = L
    return L


def resident_plan_host(row_ptr, workgroups, max_quads=15, lane_fill=0.90, no_stream=False, stream_cost=1.5):
    """avs_resident_plan_host (libavs_probe.so, no GPU): the CU-resident loop's lanes and first workgroup split for host row pointers.
    Returns (info, lanes) -- lanes: dict of row0, meta, stream_quads (info.lanes entries each), wl, wr (workgroups + 1); None when refused."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    n = len(rp) - 1
    row0, meta, quads = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    wl, wr = np.zeros(workgroups + 1, np.int32), np.zeros(workgroups + 1, np.int32)
    info = ResidentHostPlanInfo()
    check(load_probe().avs_resident_plan_host(n, rp.ctypes.data, workgroups, max_quads, lane_fill, int(no_stream), stream_cost, row0.ctypes.data,
                                              meta.ctypes.data, quads.ctypes.data, wl.ctypes.data, wr.ctypes.data, C.byref(info)))
    if info.refused:
        return info, None
    L = int(info.lanes)
    return info, {"row0": row0[:L], "meta": meta[:L], "stream_quads": quads[:L], "wl": wl, "wr": wr}


def prepass_plan_host(res, desired_levels, cut_axis=0, cuts=None, rank=0):
    """avs_prepass_plan_host (libavs_probe.so, no GPU): the plan of a pre-pass run on an octree grid `res`; cuts (world + 1 entries): the
    slab-local plan of `rank`.  Returns a dict: levels, the ranges win / nl / v / p1 as (lo, hi) arrays of `levels` entries, and the tile
    layout level_tile0 [4][MAX_LEVELS + 1], tile0_of [4][MAX_LEVELS][3], seg [5], n_exchange."""
    n = np.ascontiguousarray(res, dtype=np.int32)
    c = None if cuts is None else np.ascontiguousarray(cuts, dtype=np.int32)
    info = PrepassPlanInfo()
    check(load_probe().avs_prepass_plan_host(n.ctypes.data, desired_levels, cut_axis, None if c is None else c.ctypes.data,
                                             1 if c is None else len(c) - 1, rank, C.byref(info)))
    L = int(info.levels)
    out = {r: (np.array(getattr(info, r + "_lo"))[:L], np.array(getattr(info, r + "_hi"))[:L]) for r in ("win", "nl", "v", "p1")}
    out.update(levels=L, level_tile0=np.array(info.level_tile0), tile0_of=np.array(info.tile0_of), seg=np.array(info.seg),
               n_exchange=int(info.n_exchange))
    return out


def phase_loop_report():
    """avs_phase_loop_info (libavs_probe.so): the launch-per-phase loop's record of this thread's last solve through that library"""
    rep = PhaseLoopReport()
    check(load_probe().avs_phase_loop_info(C.byref(rep)))
    return rep


def brick_form_limits():
    """avs_brick_form_probe's limits-only call (libavs_probe.so, no GPU): the constants the brick form and its kernel were compiled with"""
    info = BrickFormInfo()
    check(load_probe().avs_brick_form_probe(0, 0, None, None, None, None, 0, 0, 0, 0, None, None, 0, 0, 0, None, None, 0, C.byref(info), None, 0, None))
    return info


def dist_plan_limits():
    """avs_dist_plan_probe's limits-only call (libavs_probe.so, no GPU): the constants the device partition planners were compiled with"""
    info = DistPlanInfo()
    check(load_probe().avs_dist_plan_probe(0, None, None, C.byref(info), None))
    return info


def dist_plan_probe(mode, row_ptr, col, val, rank, world, *, dof=None, perm=None, levels=1, cut_axis=0, extent=1, owner=None, dom=None,
                    split=0, send_capacity=None):
    """avs_dist_plan_probe on torch DEVICE tensors (int32 row_ptr / col / dof [n, 4] / perm / dom, float64 val, uint8 owner).  Returns
    (info, arrays): the plan's arrays as numpy arrays cut to their sizes (weights / plane_owner / owner in PLAN mode, local_ref / rhs_local in
    TAIL mode).  Raises AvsError on a refusal."""
    n = int(row_ptr.numel()) - 1
    nnz = int(col.numel())
    extent_planes = 65535
    send_capacity = (n * max(world - 1, 1) + 1) if send_capacity is None else send_capacity
    a = dict(weights=np.zeros(extent_planes, np.int64), plane_owner=np.zeros(extent_planes, np.int32), owner=np.zeros(n + 1, np.uint8),
             own_global=np.zeros(n + 1, np.int32), halo_global=np.zeros(n + 1, np.int32), row_ptr_local=np.zeros(n + 2, np.int32),
             col_local=np.zeros(nnz + 1, np.int32), val_local=np.zeros(nnz + 1, np.float64), send_idx=np.zeros(send_capacity, np.int32),
             peers=np.zeros(32, np.int32), send_counts=np.zeros(32, np.int32), recv_counts=np.zeros(32, np.int32),
             tiles_int=np.zeros(n + 1, np.int32), tiles_bnd=np.zeros(n + 1, np.int32), local_ref=np.zeros(n + 1, np.int32),
             rhs_local=np.zeros(n + 1, np.float64))
    ptr = lambda t: None if t is None else t.data_ptr()
    inp = DistPlanInput(n=n, row_ptr=ptr(row_ptr), col=ptr(col), val=ptr(val), dof=ptr(dof), perm=ptr(perm), owner=ptr(owner), dom=ptr(dom),
                        n_dom=0 if dom is None else int(dom.numel()), levels=levels, cut_axis=cut_axis, extent=extent, split=int(split),
                        rank=rank, world=world)
    out = DistPlanOutput(row_capacity=n + 1, nnz_capacity=nnz + 1, send_capacity=send_capacity, plane_capacity=extent_planes,
                         **{k: v.ctypes.data for k, v in a.items()})
    info = DistPlanInfo()
    check(load_probe().avs_dist_plan_probe(mode, C.byref(inp), C.byref(out), C.byref(info), None))
    sizes = dict(weights=info.nplanes, plane_owner=info.nplanes, owner=n, own_global=info.n_own, halo_global=info.n_halo,
                 row_ptr_local=info.n_own + 1, col_local=info.nnz_local, val_local=info.nnz_local, send_idx=info.n_send, peers=info.n_peers,
                 send_counts=info.n_peers, recv_counts=info.n_peers, tiles_int=info.n_tiles_int, tiles_bnd=info.n_tiles_bnd,
                 local_ref=info.n_own + info.n_halo, rhs_local=info.n_own)
    res = {k: v[:sizes[k]].copy() for k, v in a.items()}
    for k in (("local_ref", "rhs_local") if mode == DIST_PLAN_PROBE_PLAN else ("weights", "plane_owner", "owner")):
        del res[k]
    return info, res


def check(status):
    if status != OK:
        msgs = [m for m in (l.avs_last_error().decode("utf-8", "replace") for l in (_lib, _probe_lib) if l is not None) if m]
        raise AvsError(status, " | ".join(dict.fromkeys(msgs)) or "(no message)")


def ptr_of(buf):
    """(pointer, memspace) of a numpy array or a torch tensor (contiguous)."""
    if buf is None:
        return None, MEM_HOST
    if isinstance(buf, np.ndarray):
        if not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("numpy buffer must be C contiguous")
        return buf.ctypes.data, MEM_HOST
    # torch tensor
    if not buf.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return buf.data_ptr(), (MEM_DEVICE if buf.is_cuda else MEM_HOST)


# --------------------------------------------------------------------------------------------
# host-side partition planner (no GPU needed)
# --------------------------------------------------------------------------------------------
def plan_owners(dof_table, row_ptr, levels, cut_axis, extent_fine, world_size):
    """owner rank per velocity DOF (spatial slabs balanced by nnz)."""
    L = load()
    tab = np.ascontiguousarray(dof_table, np.int32)
    rp = np.ascontiguousarray(row_ptr, np.int32)
    n = len(rp) - 1
    owner = np.empty(n, np.int32)
    check(L.avs_plan_owners(n, tab.ctypes.data, rp.ctypes.data, levels, cut_axis, extent_fine, world_size,
                            owner.ctypes.data))
    return owner


def plan_create(row_ptr, col, owner, rank, world_size):
    """dict with the local structures of `rank` (see avs_plan_get_arrays)."""
    L = load()
    rp = np.ascontiguousarray(row_ptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    ow = np.ascontiguousarray(owner, np.int32)
    h = C.c_void_p()
    check(L.avs_plan_create(len(rp) - 1, rp.ctypes.data, cl.ctypes.data, ow.ctypes.data, rank, world_size, C.byref(h)))
    try:
        sz = PlanSizes()
        check(L.avs_plan_get_sizes(h, C.byref(sz)))
        a = dict(own_global=np.empty(sz.n_own, np.int32), halo_global=np.empty(sz.n_halo, np.int32),
                 row_ptr_local=np.empty(sz.n_own + 1, np.int32), col_local=np.empty(sz.nnz_local, np.int32),
                 val_src=np.empty(sz.nnz_local, np.int32), peers=np.empty(sz.n_peers, np.int32),
                 send_counts=np.empty(sz.n_peers, np.int32), recv_counts=np.empty(sz.n_peers, np.int32),
                 send_idx=np.empty(sz.n_send, np.int32))
        check(L.avs_plan_get_arrays(h, *[a[k].ctypes.data for k in
                                         ("own_global", "halo_global", "row_ptr_local", "col_local", "val_src",
                                          "peers", "send_counts", "recv_counts", "send_idx")]))
    finally:
        L.avs_plan_destroy(h)
    return a
