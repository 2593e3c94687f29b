/*
 * avs.h -- C ABI of the MI355X-native adaptive variational viscosity hot path.
 *
 * Drop-in boundary.  The reference is a Houdini GAS micro-solver whose only
 * entry point is HDK_AdaptiveViscosity::solveGasSubclass (HDK_AdaptiveViscosity.cpp:126,
 * "cpp:" below).  The proprietary HDK cannot be compiled against here, so the seam sits
 * INSIDE that function: everything between cpp:418 ("Precompute stress gradients") and
 * cpp:653 (end of "Solve Linear System") is replaced by the calls declared in this header.
 * INTEGRATION.md shows the shim a maintainer adds on the Houdini side.
 *
 * Conventions
 *   - plain C types only; the library never throws; every call returns avs_status and
 *     avs_last_error() gives a thread-local message for the last failure.
 *   - all grids are dense, x fastest ("i + rx*(j + ry*k)"), with the sample resolutions of
 *     SIM_RawField::init (HDK_Utilities.h:13-16; cpp:314-321, 370-392):
 *       centre (nx,ny,nz)>>level; face a: +1 on a; edge a: +1 on the two other axes.
 *     HDK's exint (int64) index voxels are int32 here, fp32 label voxels are int8.
 *   - pointers are host or device memory as told by avs_memspace; the library copies on
 *     every set_* (the caller keeps ownership, as Houdini does: cpp:29-34, no state survives).
 *   - one avs_ctx is used by one host thread at a time; different contexts are independent.
 *   - base resolution must be a power of two per axis (the reference pads to powers of two,
 *     HDK_OctreeGrid.cpp:18-24; power-of-two input means no padding).
 */
#ifndef AVS_H
#define AVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVS_MAX_LEVELS 8
#define AVS_EDGE_STENCIL_CAP 32   /* getEdgeStressFaces emits <= 4 slots x 8 faces, cpp:1789-1907 */
#define AVS_CENTER_STENCIL_CAP 8  /* getCenterStressFaces emits <= 2 x 4 faces, cpp:1925-1962 */
#define AVS_EDGE_BOUNDARY_CAP 4
#define AVS_CENTER_BOUNDARY_CAP 2

typedef enum {
    AVS_OK = 0,
    AVS_EINVAL = 1,    /* bad argument / inconsistent inputs (reference: addError + return false, cpp:152-229) */
    AVS_ENOMEM = 2,
    AVS_EHIP = 3,      /* a HIP runtime call failed */
    AVS_ERCCL = 4,     /* an RCCL call failed */
    AVS_EINTERNAL = 5, /* a reference assert() would have fired (e.g. foundSelf, cpp:2436) */
    AVS_ESTATE = 6     /* call sequence violated (e.g. solve before assemble) */
} avs_status;

typedef enum { AVS_MEM_HOST = 0, AVS_MEM_DEVICE = 1 } avs_memspace;

/* HDK_OctreeGrid::OctreeCellLabel, HDK_OctreeGrid.h:33-39 */
typedef enum { AVS_INACTIVE = 0, AVS_ACTIVE = 1, AVS_UP = 2, AVS_DOWN = 3 } avs_cell_label;

/* index sentinels, HDK_Utilities.h:18-21; values >= 0 are DOF / stress ids */
#define AVS_UNASSIGNED (-1)
#define AVS_SOLIDBOUNDARY (-2)
#define AVS_OUTSIDE (-3)

/* index pyramids created at cpp:337-393 */
typedef enum {
    AVS_INDEX_VELOCITY = 0, /* octreeVelocityIndices[level][axis]  (face lattice) */
    AVS_INDEX_EDGE = 1,     /* edgeStressIndices[level][axis]      (edge lattice) */
    AVS_INDEX_CENTER = 2    /* centerStressIndices[level]          (centre lattice; axis ignored) */
} avs_index_kind;

/* fp32 level-0 fields read by the hot path */
typedef enum {
    AVS_FIELD_CENTER_WEIGHTS = 0, /* centerIntegrationWeights (cpp:239)            centre */
    AVS_FIELD_EDGE_WEIGHTS = 1,   /* edgeIntegrationWeights[axis] (cpp:240)        edge a */
    AVS_FIELD_FACE_WEIGHTS = 2,   /* "faceWeights" vector field (cpp:144)          face a */
    AVS_FIELD_VISCOSITY = 3,      /* "viscosity" (cpp:203)                         centre */
    AVS_FIELD_DENSITY = 4,        /* GAS_NAME_DENSITY (cpp:218)                    centre */
    AVS_FIELD_VELOCITY = 5,       /* GAS_NAME_VELOCITY component (cpp:139)         face a */
    AVS_FIELD_SOLID_VELOCITY = 6  /* GAS_NAME_COLLISIONVELOCITY component (cpp:142) face a */
} avs_field_kind;

typedef struct {
    int32_t nx, ny, nz;             /* level-0 resolution, powers of two */
    double dx;                      /* level-0 voxel size (getVoxelSize().maxComponent(), cpp:242) */
    double dt;                      /* timestep (cpp:130) */
    int32_t levels;                 /* octreeLabels.getOctreeLevels() (cpp:275), 1..AVS_MAX_LEVELS */
    int32_t use_enhanced_gradients; /* getUseEnhancedGradients() (cpp:438) */
    int32_t device;                 /* HIP device ordinal */
    void *stream;                   /* hipStream_t to enqueue on; NULL = the library creates one */
    /* Resolution of the simulation grid the level-0 SCALAR fields live on (weights, viscosity, density, velocities),
     * i.e. before HDK_OctreeGrid::init stretched the octree grid to powers of two (oct.cpp:13-24).  0 = nx, ny, nz.
     * Labels and index pyramids always use nx, ny, nz.  Samples of the padded lattice outside this grid belong to
     * INACTIVE cells (oct.cpp:375-379) and are never read by an active row; the library fills them (viscosity /
     * density by border replication, everything else with 0).  The pre-pass takes the same field_n* in its own descriptor;
     * avs_set_regular_index_field / avs_transfer_to_regular_grid exchange arrays on the simulation grid's face lattices. */
    int32_t field_nx, field_ny, field_nz;
    /* AVS_PRECISION_F64 (0, default): SolveType = fpreal64, the build the reference ships.  AVS_PRECISION_F32: the system the
     * reference builds with USESINGLEPRECISION (util.h:25-37: SolveType = fpreal32): every triplet narrowed to float where
     * Eigen::Triplet<SolveType> is constructed (cpp:2447, 2768), duplicates summed in float (setFromTriplets, cpp:613-614), the
     * right-hand side updated in float steps (cpp:2456, 2772), the initial guess narrowed at its store (cpp:2371).  Matrix, rhs and
     * x0 are then float VALUES in the same fp64 arrays.  Single-GPU solves can iterate on FLOAT vectors with float scalars, as Eigen's
     * float CG does (round 5; dot products: a thread's terms in float, everything across threads in double -- Eigen's vectorised
     * reduction order is not reproduced): AVS_OPTION_F32_VECTORS = 1 always, -1 (default) for systems the CU-resident loop does not
     * take.  Partitioned solves (avs_dist_solve) iterate on float vectors in their single-reduction loops with
     * AVS_OPTION_DIST_F32_VECTORS = 1, over both transports; by default, and always with AVS_DIST_CG=standard and in paranoid mode,
     * they iterate in fp64 on the float system (at least as accurate, same stopping rule).  The CU-resident loop (single GPU and between
     * ranks) iterates on float vectors with AVS_OPTION_RESIDENT_F32 = 1, in fp64 otherwise.
     * The solution is a float vector either way (Eigen::VectorXf). */
    int32_t precision;
} avs_desc;
enum { AVS_PRECISION_F64 = 0, AVS_PRECISION_F32 = 1 };

typedef struct {
    int32_t iterations; /* solver.iterations() (cpp:629) */
    int32_t converged;  /* 1 if |r|^2 < tol^2 |b|^2 was reached; non-convergence is NOT an error (cpp:645-652) */
    double error;       /* solver.error() = sqrt(|r|^2/|b|^2) (cpp:630) */
    double rhs_norm2;
    int64_t n;          /* octreeVelocityDOFCount */
    int64_t nnz;
    double solve_ms;    /* HIP-event time of the PCG loop */
    double spmv_ms;     /* mean HIP-event time of one SpMV launch during this solve (0 if not sampled) */
    int32_t resident;   /* 1 = the iterations ran in the CU-resident loop (one cooperative launch: matrix words in the register files,
                           vector slices in LDS -- systems of up to ~1 M rows (~1.9 M with the rows that do not fit streamed from memory) in the packed
                           single-dictionary form, single-GPU solves and
                           partitioned solves whose rank has its GPU for itself; AVS_CG_RESIDENT=0 keeps the launch-per-phase loops) */
    int32_t cancelled;  /* 1 = avs_cancel ended the loop before convergence / max_iterations (converged is 0; x holds the last iterate) */
} avs_solve_info;

typedef struct {
    int64_t n_velocity, n_edge, n_center; /* DOF / stress counts */
    int64_t nnz;                          /* after duplicate merging */
    int64_t raw_triplets;                 /* before merging (= size of the reference's triplet list) */
    double stencil_ms, guess_ms, system_ms, csr_ms; /* HIP-event times of the phases */
} avs_assembly_info;

typedef struct avs_ctx avs_ctx;

const char *avs_last_error(void);
const char *avs_version(void);
/* ABI revision of this header: bumped whenever a struct layout or the set of exported entries changes (2: round 5 -- avs_matrix_format
 * carries struct_size, avs_solve_info.cancelled, avs_cancel; the measurement entries moved to libavs_probe.so in round 4).
 * Purely additive since (no revision): the entry avs_sample_velocity.
 * Purely additive since (no revision): the entries avs_get_octree_cells and avs_prepass_get_octree_cells.
 * Purely additive since (no revision): the entries avs_check_octree and avs_prepass_check_octree.
 * Purely additive since (no revision): the entries avs_check_csr and avs_check_system.
 * Purely additive since (no revision): the entries avs_check_stress_indices and avs_prepass_check_stress_indices.
 * Purely additive since (no revision): the entries avs_get_strain_rates and avs_get_shear_rate_field.
 * Purely additive since (no revision): the entries avs_check_solution and avs_check_csr_solution.
 * Purely additive since (no revision): the entries avs_estimate_spectrum and avs_estimate_csr_spectrum.
 * Purely additive since (no revision): the entry avs_apply_viscosity_model.
 * Purely additive since (no revision): the entries avs_prepass_set_option, avs_prepass_set_refinement, avs_prepass_get_refinement and
 *   avs_prepass_get_refinement_info.
 * Purely additive since (no revision): the option AVS_PREPASS_OPTION_APPLY_SOLID_WEIGHTS and the entry avs_prepass_get_solid_weights_info. */
#define AVS_ABI_VERSION 2
int32_t avs_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Context.  Replaces the stack-allocated temporaries of solveGasSubclass (cpp:429-470, 507-551).
 * ---------------------------------------------------------------------------------------- */
avs_status avs_create(const avs_desc *desc, avs_ctx **out);
void avs_destroy(avs_ctx *ctx);

/* ------------------------------------------------------------------------------------------
 * Inputs of the hot path (produced by cpp:233-416 in the reference).
 * ---------------------------------------------------------------------------------------- */
/* octreeLabels.getGridLabels(level), HDK_OctreeGrid.h:144-148 */
avs_status avs_set_labels(avs_ctx *ctx, int32_t level, const int8_t *labels, avs_memspace where);
/* one grid of the three index pyramids, cpp:337-393 */
avs_status avs_set_index_field(avs_ctx *ctx, avs_index_kind kind, int32_t level, int32_t axis,
                               const int32_t *indices, avs_memspace where);
/* octreeVelocityDOFCount / edgeStressDOFCount / centerStressDOFCount, cpp:355-357, 395-408.
 * Validated against the uploaded grids (max id + 1). */
avs_status avs_set_dof_counts(avs_ctx *ctx, int64_t n_velocity, int64_t n_edge, int64_t n_center);
/* data == NULL selects the constant-field fast path (field()->isConstant, cpp:2090, 2248, 2501) */
avs_status avs_set_scalar_field(avs_ctx *ctx, avs_field_kind kind, int32_t axis, const float *data,
                                float constant, avs_memspace where);

/* ------------------------------------------------------------------------------------------
 * Hot path part 1: assembly (cpp:418-594 + setFromTriplets cpp:613-614).
 * avs_assemble runs all phases; the single phases are exported for parity tests and for
 * hosts that want Houdini perf-monitor scopes per phase (cpp:441, 473, 516, 554).
 * ---------------------------------------------------------------------------------------- */
avs_status avs_build_stencils(avs_ctx *ctx);      /* buildEdgeStressStencils + buildCenterStress{Stencils,Weights}, cpp:443-498 */
avs_status avs_build_initial_guess(avs_ctx *ctx); /* buildVelocityMapping, cpp:518-528 */
avs_status avs_build_system(avs_ctx *ctx);        /* buildOctreeSystemFromStencils + triplet merge, cpp:577-593, 613-614 */
avs_status avs_assemble(avs_ctx *ctx, avs_assembly_info *info /* may be NULL */);

/* ------------------------------------------------------------------------------------------
 * Hot path part 2: solve.  Eigen::ConjugateGradient<SparseMatrix<SolveType>, Lower|Upper>
 * with DiagonalPreconditioner, solveWithGuess(rhs, restrictedVelocity) (cpp:618-630).
 * ---------------------------------------------------------------------------------------- */
avs_status avs_solve(avs_ctx *ctx, double tolerance, int32_t max_iterations, avs_solve_info *info);
/* User interrupt: the reference polls UT_Interrupt::opInterrupt() inside its loops (cpp:2528; HDK_OctreeGrid.cpp:584-588).  Callable from
 * ANY thread while another thread is inside avs_solve / avs_dist_solve on the same context: the running loop ends at its next poll of
 * the device state (every 32 iterations of the launch-per-phase loops; the CU-resident loop, one cooperative launch of at most
 * max_iterations x ~20-70 us, cannot be interrupted: it runs to its end, and the request is consumed when it returns -- reported as
 * cancelled = 1, converged = 0 if the launch stopped at max_iterations without converging, otherwise the solve is simply done), the solve
 * returns AVS_OK with converged = 0 and cancelled = 1, and the request is consumed.  A request that is already pending when avs_solve
 * starts skips the CU-resident loop: the launch-per-phase loop consumes it at its first poll (0 iterations, cancelled = 1).  A request
 * that finds no solve running cancels the NEXT one -- a host whose watcher thread may call avs_cancel right after the solve returned
 * calls avs_cancel_clear once the watcher has been joined (shim/HDK_AdaptiveViscosity_avs.cpp does).  In a partitioned solve every rank
 * must be cancelled (the ranks leave the loop in the same iteration: the request travels with the CG sums). */
avs_status avs_cancel(avs_ctx *ctx);
avs_status avs_cancel_clear(avs_ctx *ctx);   /* drop a pending request (no solve may be running on the context) */

/* Solver options of the context (set any time before avs_solve / avs_dist_solve; the default is what the USEEIGEN build does).
 * AVS_OPTION_PRECONDITIONER: AVS_PRECONDITIONER_JACOBI (0, default: Eigen's DiagonalPreconditioner, cpp:618) or
 * AVS_PRECONDITIONER_NONE (1): plain CG, what the build WITHOUT USEEIGEN asks of HDK's UT_SparseMatrixRowT::solveConjugateGradient
 * (cpp:638-642: the preconditioner argument is nullptr).  That routine is closed source: the recurrence is standard CG, the stopping
 * rule used here stays Eigen's (|r|^2 < tol^2 |b|^2), and the result is only pinned to that extent. */
typedef enum {
    AVS_OPTION_PRECONDITIONER = 0,
    AVS_OPTION_RESIDENT_LOOP = 1, /* 1 (default): the CU-resident PCG loop where a system fits the chip; 0: always the launch-per-phase loops */
    AVS_OPTION_TRANSPORT = 2,     /* multi-GPU: AVS_USE_TRANSPORT_AUTO (direct after its connect-time self-test, else RCCL), _RCCL, _DIRECT */
    AVS_OPTION_PARANOID = 3,      /* multi-GPU: 1 = every round's halo segments are re-added by the reader and compared with the sender's checksum */
    AVS_OPTION_GRAPH_REPLAY = 4,  /* 1 (default): chunks of iterations replay a captured hipGraph */
    AVS_OPTION_BRICK_FORM = 5,    /* brick-structured SpMV form: AVS_BRICK_AUTO (systems of >= 2 M rows, kept where the tiles are full enough -- a
                                   * structural rule, so the same input always runs the same kernel), _NEVER, _ALWAYS, _TUNE (auto, decided by timing
                                   * both forms at the assembly: host-synchronous and not reproducible from run to run); takes effect at the next avs_assemble */
    AVS_OPTION_FUSED_SCALAR_STEPS = 6, /* 1 (default): the CG scalar steps ride in the vector kernels; 0: one reduction launch per step */
    AVS_OPTION_RELOAD_ENVIRONMENT = 7, /* any value: take the AVS_* environment variables again (they are read once, at avs_create; tools and tests) */
    AVS_OPTION_F32_VECTORS = 8,   /* AVS_PRECISION_F32 contexts, single-GPU solves: 1 = the iteration runs on float vectors with float scalars --
                                   * SolveType = fpreal32 through Eigen::ConjugateGradient (util.h:25-37, cpp:613-630) --; 0 = fp64 iteration on
                                   * the float system; -1 (default) = float vectors where the system is too large for the CU-resident loop
                                   * (the bandwidth of the vectors is what an iteration costs there), the resident fp64 loop where it fits the
                                   * chip (faster).  With AVS_OPTION_RESIDENT_F32 = 1, -1 and 1 both run the resident loop on float vectors where
                                   * it takes the system.  Takes effect at the next avs_assemble (the brick form's walk is laid out for the kernel
                                   * that will run). */
    AVS_OPTION_FUSED_VECTOR_UPDATE = 9, /* single-GPU launch-per-phase loop: r -= alpha t and x += alpha p ; p = z + beta p as ONE launch with a grid barrier
                                   * in between -- the new r stays in registers / LDS, 7.25 n instead of 8.5 n doubles per iteration; same sums in the
                                   * same order: iteration counts and solution bits do not depend on it.  0 never, 1 wherever a system qualifies
                                   * (>= 524,288 and <= 8,388,608 rows, a device with >= 256 CUs), -1 (the default) only systems larger than the
                                   * Infinity Cache whose SpMV leaves at most 4096 partial sums (the launch then takes the alpha step as well).
                                   * A barrier that is not passed within AVS_PCG_FUSED_TIMEOUT_MS (2000; the GPU shared with other work) redoes
                                   * the solve with the two launches.  Environment: AVS_PCG_FUSE_VECTORS. */
    AVS_OPTION_DIST_F32_VECTORS = 10, /* AVS_PRECISION_F32 contexts, partitioned solves (avs_dist_solve): 1 = the single-reduction loops of both
                                   * transports iterate on float vectors with float scalars, as the single-GPU AVS_OPTION_F32_VECTORS = 1 does (the
                                   * CU-resident loop between ranks is then skipped, unless AVS_OPTION_RESIDENT_F32 = 1 runs it on float vectors);
                                   * 0 (default) = fp64 iteration on the float system.  AVS_DIST_CG=standard and paranoid mode keep their fp64 loops.
                                   * No effect on AVS_PRECISION_F64 contexts.  Takes effect at the next avs_dist_partition / avs_dist_assemble (the
                                   * local brick form's walk is laid out for the kernel that will run).  Environment: AVS_DIST_F32_VECTORS. */
    AVS_OPTION_RESIDENT_F32 = 12, /* (11 is not assigned: avs_set_solver_option rejects it.)  AVS_PRECISION_F32 contexts: 1 = the CU-resident
                                   * loop iterates on float vectors with float scalars (float vector slices, remote columns and tables in LDS, float row sums, a thread's terms summed in float, everything across
                                   * threads / workgroups / ranks in double) where it takes a system that would otherwise iterate on float vectors:
                                   * single-GPU solves with AVS_OPTION_F32_VECTORS = -1 or 1, partitioned solves with AVS_OPTION_DIST_F32_VECTORS = 1
                                   * (the latter latched at the next avs_dist_partition / avs_dist_assemble).  0 (default) = as before: the resident
                                   * loop stays fp64, and float-vector solves use the launch-per-phase / single-reduction loops.  With
                                   * AVS_OPTION_F32_VECTORS = 0, AVS_DIST_CG=standard or paranoid mode nothing changes.  Reported through
                                   * avs_solve_info.resident and avs_matrix_format.float_vectors.  No effect on AVS_PRECISION_F64 contexts.
                                   * Environment: AVS_RESIDENT_F32. */
    AVS_OPTION_RESIDENT_LOCAL_TABLES = 13, /* 1 = the CU-resident loop also takes a matrix WITHOUT one dictionary of <= 1,023 values (a viscosity or density
                                   * field, a curved boundary: tile-local tables, column windows, 6-B or plain 12-B words at the assembly): the plan
                                   * gives every workgroup -- or, where the 25-bit matrix word has no room for a workgroup's code bits, every wave --
                                   * its own value table, the distinct bit patterns of the rows it holds in ascending order, taken from the plain CSR
                                   * values; the inverse diagonal is read per row.  Same row sums and the same recurrences as the launch-per-phase
                                   * loops.  Everything else that keeps a system off the chip (rows, LDS, a shared GPU, a pending cancel,
                                   * AVS_OPTION_RESIDENT_LOOP = 0) still applies; a plan that does not fit says which quantity did not
                                   * (AVS_CG_RESIDENT_VERBOSE=1) and the solve runs the launch-per-phase loop as before.  0 (default) = such systems
                                   * are not planned at all.  Matrices the resident loop takes today run the ordinary plan either way.  Both vector
                                   * types (float: with AVS_OPTION_RESIDENT_F32).  Reported through avs_solve_info.resident.  Read at the next
                                   * solve: switching it plans again.  Environment: AVS_RESIDENT_LOCAL_TABLES. */
    AVS_OPTION_MIXED_PRECISION = 14, /* AVS_PRECISION_F64 contexts, single-GPU solves: 1 = a solve that would run the fp64 launch-per-phase loop iterates
                                   * on float vectors instead (r, p, A p and a correction xf: 4 B per row and stream; the matrix values and every
                                   * row sum stay fp64, the sum is rounded to float once; alpha, beta, the dot products and the threshold stay
                                   * fp64), and every 32 iterations -- and whenever the float recurrence claims convergence -- the correction is
                                   * folded into the fp64 solution and the residual replaced by b - A x computed in fp64 ("reliable updates"; the
                                   * search direction is kept).  The answer and the stopping test are fp64: avs_solve_info.error and .converged
                                   * come from the last fp64 residual, .iterations counts the float iterations.  Systems the CU-resident loop
                                   * takes keep it (fp64; AVS_OPTION_RESIDENT_LOOP = 0 sends them here).  Both preconditioner settings.  0 (default)
                                   * = nothing changes.  No effect on AVS_PRECISION_F32 contexts or on avs_dist_solve.  Reported through
                                   * avs_matrix_format.float_vectors and .reliable_updates.  Takes effect at the next avs_assemble (the brick form's
                                   * walk is laid out for the kernel that will run).  Environment: AVS_MIXED_PRECISION. */
    AVS_OPTION_DIST_MIXED_PRECISION = 15 /* AVS_PRECISION_F64 contexts, partitioned solves (avs_dist_solve): 1 = the single-reduction loops of both
                                   * transports iterate on float vectors (r, u, A u, p, s and a correction xf) with the scheme of
                                   * AVS_OPTION_MIXED_PRECISION: matrix values, row sums (rounded to float once), dot products, alpha, beta and the
                                   * threshold stay fp64, and behind every 32 iterations -- and whenever the float recurrence claims convergence --
                                   * the correction is folded into the fp64 solution, x is exchanged in fp64 and the residual replaced by b - A x
                                   * computed in fp64; the Chronopoulos-Gear step of that iteration is taken on the true residual's sums.
                                   * avs_solve_info.error and .converged come from the last fp64 residual, .iterations counts the float
                                   * iterations, .resident is 0 (the CU-resident loop between ranks is skipped).  AVS_DIST_CG=standard, paranoid
                                   * mode, AVS_PRECISION_F32 contexts and avs_solve are not affected.  0 (default) = nothing changes.  Reported
                                   * through avs_matrix_format.float_vectors and .reliable_updates.  Read at the next avs_dist_partition /
                                   * avs_dist_assemble (the local brick form's walk is laid out for the kernel that will run).
                                   * Environment: AVS_DIST_MIXED_PRECISION. */
} avs_solver_option;
enum { AVS_USE_TRANSPORT_AUTO = 0, AVS_USE_TRANSPORT_RCCL = 1, AVS_USE_TRANSPORT_DIRECT = 2 };
enum { AVS_BRICK_AUTO = -1, AVS_BRICK_NEVER = 0, AVS_BRICK_ALWAYS = 1, AVS_BRICK_TUNE = 2 };
enum { AVS_PRECONDITIONER_JACOBI = 0, AVS_PRECONDITIONER_NONE = 1 };
avs_status avs_set_solver_option(avs_ctx *ctx, avs_solver_option option, int32_t value);

/* ------------------------------------------------------------------------------------------
 * Outputs.  avs_get_solution is what cpp:661-707 consumes (viscositySolution).
 * The others exist for parity tests.  Any pointer may be NULL to skip that array.
 * ---------------------------------------------------------------------------------------- */
avs_status avs_get_assembly_info(avs_ctx *ctx, avs_assembly_info *info);
/* storage the solver's SpMV streams for the assembled matrix (all forms are lossless: the same products
 * in the same order as plain CSR).  12 B/non-zero: fp64 value + int32 column (what Eigen holds, cpp:613);
 * 6 B: uint16 code into a table of the matrix's distinct values + int32 column; 4 B: code and column
 * packed in one word, when bits(n) + bits(table) <= 32.  With more than 2048 distinct values the 6-B form keeps one
 * dictionary per SpMV tile (tile_local_tables): the values of a 512-row tile repeat even when the matrix as a whole
 * has 10^4..10^5 distinct ones (smoothly varying viscosity), and a tile's table fits in LDS.  When code and column do not fit
 * one word directly (many values, or more than 2^25 columns) the column is stored tile-relative (column_windows): 4 B again. */
typedef struct avs_matrix_format {
    int32_t struct_size;        /* IN: sizeof(avs_matrix_format) of the caller's header -- only that many bytes are written (the struct has grown
                                 * between revisions; a caller built against an older header keeps working) */
    int32_t reordered;          /* 1 = rows/columns renumbered brick-major inside the solver */
    int32_t value_table_size;   /* distinct values; 0 = not value-indexed (> 65536 distinct values) */
    int32_t column_bits;        /* > 0 = packed form, columns in the low bits */
    int32_t bytes_per_nonzero;  /* 12, 6 or 4 */
    int32_t tile_local_tables;  /* 1 = one dictionary per 512-row SpMV tile (value_table_size = total entries, 8 B each, streamed once) */
    int32_t column_windows;     /* 1 = 4-B words code | window slot | offset: a tile's columns lie in <= 64 windows of 2^14 ids (+ 256 B per tile) */
    int32_t brick_tiles;        /* > 0 = the single-GPU loop multiplies with the brick-structured form (csrc/avs_brick.hip): rows of one 8^3
                                 * brick of fine cells stored as geometric row patterns (one 8-B descriptor per row), the rest as 4-B words */
    int32_t brick_patterns;     /* distinct row patterns of the whole matrix */
    int64_t brick_pattern_rows; /* rows stored as patterns */
    int64_t brick_bytes;        /* bytes the brick kernel streams per launch for the matrix (descriptors, runs, pattern lists, words) */
    int32_t brick_walk;         /* tile walk of the persistent workgroups: 0 one contiguous eighth of the tiles per XCD, 1 chunks dealt to the XCDs in turn */
    int32_t brick_value_codes;  /* 1 = variable-viscosity variant: the patterns carry the geometry only, every pattern row streams its own 2-B value codes
                                 * into a per-tile value table (round 5) */
    int32_t fused_vector_update; /* 1 = the last avs_solve enqueued the two vector kernels of an iteration as one launch (AVS_OPTION_FUSED_VECTOR_UPDATE) */
    int32_t fused_vector_faults; /* launches of it on this context whose grid barrier timed out (the solve was redone with the two launches) */
    int32_t float_vectors;      /* 1 = the last avs_solve or avs_dist_solve on this context iterated on float vectors (AVS_OPTION_F32_VECTORS,
                                 * AVS_OPTION_DIST_F32_VECTORS, AVS_OPTION_MIXED_PRECISION, AVS_OPTION_DIST_MIXED_PRECISION) */
    int32_t reliable_updates;   /* fp64 residual updates (x += xf, r = b - A x) of the last avs_solve or avs_dist_solve: the mixed-precision
                                 * loops (AVS_OPTION_MIXED_PRECISION, AVS_OPTION_DIST_MIXED_PRECISION); 0 for every other loop */
} avs_matrix_format;
avs_status avs_get_matrix_format(avs_ctx *ctx, avs_matrix_format *fmt);
avs_status avs_get_solution(avs_ctx *ctx, double *x, int64_t n, avs_memspace where);
avs_status avs_get_initial_guess(avs_ctx *ctx, double *x0, int64_t n, avs_memspace where);
/* hands the context a solution vector (reference DOF numbering, n_velocity entries) for the post-solve transfer: a hosted multi-GPU
 * group's host program sums the per-rank vectors of avs_dist_get_solution itself and gives every rank the whole vector back; also a
 * velocity computed elsewhere (tests: the same vector through two transfer paths).  The reference keeps its solution in `solution`
 * between cpp:645 and cpp:655-707. */
avs_status avs_set_solution(avs_ctx *ctx, const double *x, int64_t n, avs_memspace where);
avs_status avs_get_csr(avs_ctx *ctx, int32_t *row_ptr /* n+1 */, int32_t *col, double *val,
                       double *rhs, avs_memspace where);
/* SoA stencil records: entry k of stencil s lives at [k * count + s].
 * edge:   count = n_edge,     cap AVS_EDGE_STENCIL_CAP,   boundary cap AVS_EDGE_BOUNDARY_CAP
 * centre: count = 3*n_center (list id = cell id + n_center*axis, cpp:2186), weights n_center */
avs_status avs_get_edge_stencils(avs_ctx *ctx, int32_t *cnt, int32_t *idx, double *coef,
                                 int32_t *bcnt, double *bval, double *weight, avs_memspace where);
avs_status avs_get_center_stencils(avs_ctx *ctx, int32_t *cnt, int32_t *idx, double *coef,
                                   int32_t *bcnt, double *bval, double *weight, avs_memspace where);

/* ------------------------------------------------------------------------------------------
 * Post-solve transfer (SURVEY 8(f) "next #2"): what cpp:655-707 does with viscositySolution --
 * setOctreeVelocity (cpp:2779-2813), HDK_OctreeVectorFieldInterpolator (node values, T-junction
 * aware; HDK_OctreeVectorFieldInterpolator.cpp:118-845) and applyVelocitiesToRegularGrid
 * (cpp:2815-2894): the regular MAC-grid velocity Houdini reads back.
 * ---------------------------------------------------------------------------------------- */
/* regularVelocityIndices[axis] (cpp:303-329): >= 0 regular DOF, AVS_SOLIDBOUNDARY, else untouched face; on the face lattice
 * of the SIMULATION grid (field_n*, + 1 on `axis`) */
avs_status avs_set_regular_index_field(avs_ctx *ctx, int32_t axis, const int32_t *indices, avs_memspace where);
/* out_*: face lattices of the simulation grid (field_n*); faces that are not regular DOFs keep the input velocity */
avs_status avs_transfer_to_regular_grid(avs_ctx *ctx, float *out_x, float *out_y, float *out_z, avs_memspace where);
/* The same transfer as an IN-PLACE update, which is what the reference does to `vel` (cpp:655-707: only the faces named by
 * regularVelocityIndices are assigned).  vel_x/y/z: DEVICE arrays on the simulation grid's face lattices that already hold the velocity
 * field given to avs_set_scalar_field(AVS_FIELD_VELOCITY): only the faces the transfer changes are written -- on a sparse scene nine
 * tiles in ten are neither read nor written.  (Simulation grids that HDK_OctreeGrid::init had to pad are written face by face as by
 * avs_transfer_to_regular_grid.) */
avs_status avs_transfer_to_regular_grid_in_place(avs_ctx *ctx, float *vel_x, float *vel_y, float *vel_z);
/* interpolator node grids after all passes, (n+1)^3 per level: labels (0 inactive, 1 active), values fp32 */
avs_status avs_get_node_grid(avs_ctx *ctx, int32_t level, int8_t *labels, float *vx, float *vy, float *vz, avs_memspace where);
/* interpSPGrid (interp.h:140, interp.cpp:660-845) for arbitrary positions, all three components per point: the solved octree velocity
 * anywhere in the grid (particle updates, markers, render grids of another resolution or offset, probes), by the same T-junction-aware
 * trilinear / node-plus-bubble interpolation the transfer applies on the regular face lattice -- at a face position of that lattice
 * component `axis` equals the transfer's value bit for bit.  A position becomes q[a] = ((double)p[a] - origin[a]) / dx in fp64 (level-0
 * cells, dx of the avs_desc).  Positions are handled in exact index space (every index position the reference derives is q scaled by a
 * power of two, minus the lattice's half-cell offset); HDK's fp32 posToIndex round trip is not reproduced; where it would decide a tie
 * (a point lying exactly on a cell boundary) the forward cell is taken.  A point is outside when q is NaN or outside [0, n_a], or when no
 * level holds an ACTIVE cell over it (the reference asserts there): velocity 0, 0, 0 and inside = 0; nothing is read out of bounds for it.
 * Points are evaluated in caller order (no sorting); the result of a point does not depend on the others.
 * Needs a solution (avs_solve, avs_set_solution, or avs_dist_get_solution on a context that is not slab-local) and the dof tables, else
 * AVS_ESTATE; regular-grid index fields are NOT needed.  n_points == 0: AVS_OK, nothing is touched.  Slab-local contexts
 * (avs_prepass_set_slab): AVS_ESTATE.  The interpolator's node grids are kept in the context and rebuilt only after the solution, the
 * pyramids or the dof tables have changed -- sampling after a transfer of the same solution (or the reverse) runs no node pass. */
avs_status avs_sample_velocity(avs_ctx *ctx, int64_t n_points,
                               const float *positions,   /* n_points x 3, xyz interleaved, world units */
                               const double *origin,     /* 3 doubles: world position of the grid's lower corner; NULL = 0,0,0 */
                               float *velocity,          /* n_points x 3, xyz interleaved */
                               uint8_t *inside,          /* n_points, may be NULL: 1 = an ACTIVE cell contains the point */
                               avs_memspace where);

/* The octree's ACTIVE cells as points (HDK_OctreeGrid::outputOctreeGeometry, oct.cpp:245-308: the "Output Octree Geometry" / "Only Output
 * Octree" toggles, cpp:78-79, 283-294), computed on the device from the label pyramid the context holds -- labels set by avs_set_labels
 * or lent by avs_prepass_apply.  avs_prepass_get_octree_cells (below, with the pre-pass) is the same call on a pre-pass object.
 * Which cells: every cell labelled AVS_ACTIVE at every level 0 .. levels-1; whether the pyramid is a valid octree is not judged.  On a
 *   padded grid (field_n*) the cells outside the simulation grid are INACTIVE (oct.cpp:375-379) and never appear.
 * Order: the reference's sweep -- levels ascending; inside a level UT_VoxelArray tile order (16^3 tiles, x fastest, then y, then z); inside
 *   a tile x fastest, then y, then z; a lattice extent that is no multiple of 16 ends in a partial tile of the voxels that exist.
 * Values of record r: level[r] = l; ijk[3r ..] = the cell's index on its level's lattice; pscale[r] = (float)(dx * 2^l), the level's voxel
 *   size; position[3r + a] = (float)(origin[a] + (i_a + 0.5) * dx * 2^l), evaluated in fp64 and rounded once -- the convention of
 *   avs_sample_velocity (q = (p - origin) / dx).  HDK's own fp32 indexToPos arithmetic is closed source and is not reproduced.
 * Capacity protocol: *n_cells is always written, per_level[0 .. AVS_MAX_LEVELS) when non-NULL (the count per level).  capacity == 0 is a
 *   count query: the array pointers are ignored and may be NULL.  capacity >= *n_cells: exactly *n_cells records are written and nothing
 *   behind them is touched.  0 < capacity < *n_cells: AVS_EINVAL, no array element is written.  No ACTIVE cell: AVS_OK, *n_cells = 0.
 *   position, pscale, level or ijk == NULL skips that array.  The count is 64-bit; one call emits at most 2^31 - 1 cells (tile offsets
 *   are 32-bit): beyond that a count query still answers, a call with capacity > 0 returns AVS_EINVAL.
 * Memory: AVS_MEM_DEVICE arrays are written by the kernel directly (no staging copy) on the object's stream, and the call returns once the
 *   count is known -- the records are complete in stream order, so they can go straight into avs_sample_velocity on the same context;
 *   work on another stream is ordered behind the object's stream by the caller (hipDeviceSynchronize for a stream the library created).
 *   AVS_MEM_HOST arrays are staged and complete on return.  Scratch (tile counts, offsets, tile list, staging) stays in the object.
 * State: labels of every level, else AVS_ESTATE; no assembly, solve or index pyramid is needed.  Slab-local contexts and pre-passes
 *   (avs_prepass_set_slab: labels inside the rank's window only): AVS_ESTATE.  The pre-pass entry needs a completed avs_prepass_run
 *   (AVS_ESTATE otherwise); a run that found no liquid (levels == 0) gives AVS_OK and *n_cells = 0.
 * The same labels give the same bytes on every call and in every fresh object. */
avs_status avs_get_octree_cells(avs_ctx *ctx, const double *origin /* 3, NULL = 0,0,0 */, int64_t capacity,
                                float *position /* capacity x 3, xyz interleaved, world units */, float *pscale /* capacity */,
                                int32_t *level /* capacity */, int32_t *ijk /* capacity x 3; may be NULL */,
                                int64_t *n_cells, int64_t *per_level /* AVS_MAX_LEVELS, may be NULL */, avs_memspace where);

/* Is the pyramid the context holds one the hot path is defined for?  The reference's debug invariants -- HDK_OctreeGrid::unitTest
 * (oct.cpp:984-1304, called at cpp:881) and octreeVelocityUnitTest (cpp:2896-2999, called at cpp:411) -- evaluated on the device over the
 * label pyramid and the velocity index pyramid as they lie there (set by avs_set_labels / avs_set_index_field or lent by
 * avs_prepass_apply: checked in place).  avs_prepass_check_octree (below, with the pre-pass) is the same call on a pre-pass object.
 * Nothing else in the library calls it, and it changes nothing: every other entry behaves as without it.
 * L = levels, the lattices are n >> l; a cell outside its lattice counts as INACTIVE.  violations[r] = lattice entries that break rule r
 * at least once (64-bit); every rule is evaluated independently of the others:
 *   0 LABEL_VALUE  every label of every level is 0 .. 3.
 *   1 COLUMN       (oct.cpp:984-1080) a level-0 cell and its ancestors at levels 1 .. L-1, ascending.  INACTIVE: every ancestor is
 *                  INACTIVE or DOWN and no INACTIVE follows a DOWN.  ACTIVE: every ancestor is DOWN.  UP: the ancestors read UP* ACTIVE
 *                  DOWN* with exactly one ACTIVE (an UP column without an ACTIVE ancestor violates; the reference lets it pass).  Any
 *                  other level-0 label (DOWN) violates.  Entries: level-0 cells.
 *   2 UP           (oct.cpp:1082-1160) an UP cell at level l: l < L-1, all eight cells of its sibling block are UP, every in-lattice face
 *                  neighbour is ACTIVE or UP.
 *   3 ACTIVE       (oct.cpp:1162-1248, as its comment states it: the reference's loop body never runs, its guard `!passed` is false on
 *                  entry) an ACTIVE cell at level l and each in-lattice face neighbour.  Neighbour DOWN: l > 0 and the neighbour's four
 *                  children on the shared face are ACTIVE.  Neighbour UP: l < L-1 and the neighbour's parent is ACTIVE.
 *   4 INDEX_VALUE  every velocity index is >= AVS_OUTSIDE and < n_velocity.
 *   5 FACE         (cpp:2925-2965) a face with id >= 0 at level l and the labels of its backward / forward cell: ACTIVE / ACTIVE, or
 *                  ACTIVE / UP (or UP / ACTIVE) with l < L-1 and the UP cell's parent ACTIVE.
 *   6 SENTINEL     (cpp:2966-2973) AVS_OUTSIDE and AVS_SOLIDBOUNDARY occur at level 0 only.
 *   7 NUMBERING    every id in [0, n_velocity) occurs exactly once over all levels and axes (entries: the ids that occur 0 times or more
 *                  than once; ids out of range are rule 4's).  The reference does not assert it; a repeated id corrupts the dof table.
 * what: AVS_CHECK_LABELS = rules 0 .. 3, AVS_CHECK_VELOCITY_INDICES = rules 4 .. 7, or both; any other bit: AVS_EINVAL.  what == 0: AVS_OK,
 *   passed = 1, nothing is launched.  Rules that were not asked for report 0 violations.
 * first_*: the violating entry that comes first by (rule, level, axis, linear index "i + rx*(j + ry*k)" in its lattice); -1 everywhere when
 *   passed.  Label rules report axis 0, rule 1 level 0; rule 7 reports level 0, axis 0 and first_ijk = (id, 0, 0).
 * struct_size: IN, as in avs_matrix_format -- only that many bytes of the report are written.
 * State: AVS_CHECK_LABELS needs the labels of every level; AVS_CHECK_VELOCITY_INDICES in addition the velocity lattices of every level and
 *   axis and the dof counts (avs_set_dof_counts); anything missing: AVS_ESTATE.  Slab-local contexts and pre-passes: AVS_ESTATE.  The
 *   pre-pass entry needs a completed avs_prepass_run; a run that found no liquid (levels == 0) gives passed = 1.
 * The work is enqueued on the object's stream and the call returns once the report is on the host; scratch (one int32 per velocity id, the
 *   raw report) stays in the object.  The same lattices give the same report on every call. */
enum { AVS_CHECK_LABELS = 1, AVS_CHECK_VELOCITY_INDICES = 2 };
enum { AVS_RULE_LABEL_VALUE = 0, AVS_RULE_COLUMN = 1, AVS_RULE_UP = 2, AVS_RULE_ACTIVE = 3,
       AVS_RULE_INDEX_VALUE = 4, AVS_RULE_FACE = 5, AVS_RULE_SENTINEL = 6, AVS_RULE_NUMBERING = 7, AVS_OCTREE_RULES = 8 };
typedef struct avs_octree_check {
    int32_t struct_size;                   /* IN: sizeof(avs_octree_check) of the caller's header */
    int32_t passed;                        /* 1 = no rule that was asked for is violated */
    int64_t violations[AVS_OCTREE_RULES];
    int32_t first_rule, first_level, first_axis, first_ijk[3];
} avs_octree_check;
avs_status avs_check_octree(avs_ctx *ctx, uint32_t what, avs_octree_check *report);

/* The same question for the two stress index pyramids (AVS_INDEX_EDGE, AVS_INDEX_CENTER), which decide which stencils avs_assemble builds
 * and where their records are stored.  The reference's debug invariants -- edgeStressUnitTest and centerStresUnitTest (cpp:3001-3298,
 * called at cpp:412-413) -- evaluated on the device over the lattices as they lie there (set by avs_set_index_field or lent by
 * avs_prepass_apply: checked in place).  avs_prepass_check_stress_indices (below, with the pre-pass) is the same call on a pre-pass object.
 * Nothing else in the library calls it, and it changes nothing: every other entry behaves as without it.
 * L = levels, cell lattices are n >> l; the edge lattice of axis a has one more entry on the two other axes b = (a+1)%3 and c = (a+2)%3, the
 * face lattice of axis f one more on f.  A cell outside its lattice reads as INACTIVE, an index outside its lattice as AVS_UNASSIGNED.
 * Values of the label and velocity pyramids are only compared with sentinels (check those with avs_check_octree).  violations[r] = lattice
 * entries that break rule r at least once (64-bit); every rule is evaluated independently of the others:
 *   0 EDGE_VALUE        every edge index is AVS_UNASSIGNED, AVS_OUTSIDE or in [0, n_edge).  AVS_SOLIDBOUNDARY violates: classification
 *                       never writes it to a stress lattice.
 *   1 EDGE_CELLS        (cpp:3037-3052) an edge e of axis a at level l with id >= 0 and the four cells around it, walked as the reference
 *                       walks them: e - 1_b - 1_c, e - 1_c, e - 1_b, e, up to the first one outside the lattice.  Every cell reached is
 *                       ACTIVE or UP.  (The reference's comment asks for all four.  Its loop, like the classification that writes the
 *                       lattice, cpp:1361-1370, leaves at the first cell outside: on the upper border plane of b an edge is decided by
 *                       its first cell alone, and liquid that reaches that border at a coarse level yields an edge with an id next
 *                       to a DOWN cell the walk never sees.  The pre-pass yields such pyramids, so the rule asserts what the reference asserts.)
 *   2 EDGE_FACES        (cpp:3054-3121) the same edges; for f in {b, c}, o the third axis, the two faces of axis f at e and e - 1_o; a face
 *                       whose o coordinate is < 0 or >= (n_o >> l) is skipped.  The velocity index v of a face: v >= 0 is fine.
 *                       AVS_SOLIDBOUNDARY or AVS_OUTSIDE: l == 0.  AVS_UNASSIGNED and e[f] odd (a T-junction inside a coarse cell): l < L-1
 *                       and the level-(l+1) cell face >> 1 is ACTIVE.  AVS_UNASSIGNED and e[f] even: l < L-1 and the level-(l+1) velocity
 *                       index of axis f at face >> 1 is not AVS_UNASSIGNED.  Any other negative value violates.
 *                       Narrower than the reference on the border of the grid, where its assert rejects what its own classification
 *                       (and the pre-pass here) writes once liquid reaches the border at a coarse level: a face on a border plane of
 *                       its lattice (f coordinate 0 or n_f >> l; never numbered, cpp:1210-1215: AVS_OUTSIDE at level 0, untouched
 *                       above) is skipped, and so is every face of an edge with e[b] == n_b >> l (rule 1's walk ends after its first
 *                       cell, so the cells beside those faces were never looked at).
 *   3 EDGE_NUMBERING    every id in [0, n_edge) occurs exactly once over all levels and axes (entries: the ids that occur 0 times or more
 *                       than once; ids out of range are rule 0's).  The reference does not assert it.
 *   4 CENTER_VALUE      rule 0 for the centre indices, against n_center.
 *   5 CENTER_LABEL      (cpp:3184) a centre with id >= 0 lies on an ACTIVE cell.
 *   6 CENTER_FACES      (cpp:3190-3231) the same centres at level l and their six faces cell + d 1_a, d in {0, 1}.  The velocity index v:
 *                       AVS_UNASSIGNED: l > 0 and the four child faces 2 face + {0,1} 1_b + {0,1} 1_c of level l-1 are all >= 0.
 *                       AVS_OUTSIDE or AVS_SOLIDBOUNDARY: l == 0.  Any other negative value violates.  A face on a border plane of its
 *                       lattice (a coordinate 0 or n_a >> l) is skipped, as in rule 2: a coarse ACTIVE cell on the border of the grid
 *                       has an UNASSIGNED face there with UNASSIGNED children, which the reference's assert rejects.
 *   7 CENTER_EDGES      (cpp:3233-3266) the same centres and their twelve edges: axis a, cell + {0,1} 1_b + {0,1} 1_c.  Only an
 *                       AVS_UNASSIGNED edge index is examined (AVS_OUTSIDE passes, as in the reference): l > 0, and for each of the two child
 *                       edges 2 edge + {0,1} 1_a of level l-1 whose index is < 0: l >= 2 and both grandchildren 2 child + {0,1} 1_a of level
 *                       l-2 are >= 0.  (Where this rule reports a violation at l == 0 or l == 1, the reference indexes level -1 or -2.)
 *   8 CENTER_NUMBERING  rule 3 over [0, n_center).
 * what: AVS_CHECK_EDGE_INDICES = rules 0 .. 3, AVS_CHECK_CENTER_INDICES = rules 4 .. 8, or both; any other bit: AVS_EINVAL.  what == 0:
 *   AVS_OK, passed = 1, nothing is launched.  Rules that were not asked for report 0 violations and are not launched.
 * first_*: the violating entry that comes first by (rule, level, axis, linear index "i + rx*(j + ry*k)" in its own lattice); -1 everywhere
 *   when passed.  Centre rules report axis 0; rules 3 and 8 report level 0, axis 0 and first_ijk = (id, 0, 0).
 * active_edges, active_centers: entries with a stored value >= 0, over all levels (and axes); 0 for a kind that was not asked for.
 * struct_size: IN, as in avs_octree_check -- only that many bytes of the report are written; below offsetof(passed) + 4 or above 4096, a
 *   NULL report: AVS_EINVAL.
 * State: AVS_CHECK_EDGE_INDICES needs the labels of every level, the velocity and edge lattices of every level and axis and the dof counts
 *   (avs_set_dof_counts); AVS_CHECK_CENTER_INDICES in addition the centre lattices; anything missing: AVS_ESTATE.  Slab-local contexts and
 *   pre-passes: AVS_ESTATE.  The pre-pass entry needs a completed avs_prepass_run; a run that found no liquid (levels == 0) gives passed = 1.
 * A pyramid that passes is one the pre-pass can have written; avs_assemble still reports on its own (AVS_EINTERNAL) the stencils the
 *   reference cannot build, such as an UNASSIGNED face beside an edge of the top level on the border of the grid.
 * The work is enqueued on the object's stream and the call returns once the report is on the host; scratch (one int32 per edge id and per
 *   centre id, the raw report) stays in the object.  The same lattices give the same report on every call. */
enum { AVS_CHECK_EDGE_INDICES = 1, AVS_CHECK_CENTER_INDICES = 2 };
enum { AVS_STRESS_RULE_EDGE_VALUE = 0, AVS_STRESS_RULE_EDGE_CELLS = 1, AVS_STRESS_RULE_EDGE_FACES = 2, AVS_STRESS_RULE_EDGE_NUMBERING = 3,
       AVS_STRESS_RULE_CENTER_VALUE = 4, AVS_STRESS_RULE_CENTER_LABEL = 5, AVS_STRESS_RULE_CENTER_FACES = 6, AVS_STRESS_RULE_CENTER_EDGES = 7,
       AVS_STRESS_RULE_CENTER_NUMBERING = 8, AVS_STRESS_RULES = 9 };
typedef struct avs_stress_check {
    int32_t struct_size;                   /* IN: sizeof(avs_stress_check) of the caller's header */
    int32_t passed;                        /* 1 = no rule that was asked for is violated */
    int64_t violations[AVS_STRESS_RULES];
    int32_t first_rule, first_level, first_axis, first_ijk[3];
    int64_t active_edges, active_centers;
} avs_stress_check;
avs_status avs_check_stress_indices(avs_ctx *ctx, uint32_t what, avs_stress_check *report);

/* The deformation of a velocity: the rate of every stress stencil, a shear rate per ACTIVE cell, the dissipation of the step, and the shear
 * rate gamma = sqrt(2 eps:eps) as a field on the simulation grid -- what a host needs to evaluate a shear-dependent viscosity mu(gamma)
 * (Carreau, Bingham, a shear-thinning melt).  Every edge stencil of avs_build_stencils is a row of the deformation-rate operator (eps_bc
 * at an edge of axis a, b = (a+1)%3, c = (a+2)%3), every centre stencil list du_a/dx_a at a cell (cpp:443-498).  Nothing else in the
 * library calls these entries, and they write nothing a later assemble, solve or transfer reads.
 * which: the velocity vector u the stencils are applied to (n_velocity entries, reference numbering).  AVS_RATES_OF_SOLUTION: the solution
 *   (avs_solve, avs_set_solution, or avs_dist_get_solution on a context that is not slab-local).  AVS_RATES_OF_INITIAL_GUESS: the
 *   restricted input velocity of avs_build_initial_guess / avs_assemble (not the partial one of avs_dist_assemble) -- what a viscosity model
 *   uses BEFORE the solve: provisional fields, avs_build_stencils, avs_build_initial_guess, avs_get_shear_rate_field, mu(gamma),
 *   avs_set_scalar_field(AVS_FIELD_VISCOSITY), avs_assemble, avs_solve (avs_apply_viscosity_model below does the two middle steps on the
 *   device).  No system has to be assembled for either.
 * Rate of a stencil s (of `count` stencils, SoA as in avs_get_edge_stencils): fp64, one rounding per operation.  acc = 0; for k = 0 ..
 *   cnt[s]-1 in stored order acc = acc + coef[k*count + s] * u[idx[k*count + s]]; then for k = 0 .. bcnt[s]-1 acc = acc + bval[k*count + s].
 *   Slots at or behind cnt / bcnt are never read.  cnt == 0 gives the sum of the boundary terms.  AVS_PRECISION_F32 contexts are
 *   evaluated the same way on the values they store.  edge_rate[e]: edge stress e; center_rate[cid + n_center*a] = eps_aa of centre cid.
 * Shear rate of the cell with centre id cid, at level l, cell C (mirrors rule 7 CENTER_EDGES of avs_check_stress_indices, the reference's
 *   statement of which edges an ACTIVE cell owns, cpp:3233-3266).  For edge axis a the four slots e = C + {0,1} 1_b + {0,1} 1_c of the
 *   level-l edge lattice of axis a, the b offset fastest.  A slot is resolved by its edge index v:
 *     v >= 0                         the rate of edge v (counted in edge_lookups[AVS_EDGE_LOOKUP_OWN]);
 *     v == AVS_UNASSIGNED and l > 0  the two children 2 e + {0,1} 1_a of level l-1, in that order.  A child with id >= 0 contributes its
 *                                    rate (..._CHILD, per child).  A child with a negative index contributes, if l >= 2, the mean of its
 *                                    grandchildren 2 child + {0,1} 1_a of level l-2 that have an id >= 0 (..._GRANDCHILD, per grandchild
 *                                    used; none: the child contributes nothing).  The slot's value is the sum of the contributing
 *                                    children in order divided by their number; no contributing child: the slot is skipped;
 *     anything else                  skipped (..._SKIPPED, per slot): AVS_OUTSIDE, AVS_UNASSIGNED at level 0, a slot without a descendant
 *                                    -- a free surface has no stress sample there.  An index outside its lattice reads as AVS_UNASSIGNED,
 *                                    an id >= n_edge as no id.
 *   m_a = the sum of the contributing slots in slot order divided by their number; no contributing slot: m_a = 0 and the pair (cell, a)
 *   is counted in empty_pairs.  A mean is (x) / 1, (x + y) / 2, ((x + y) + z) / 3, (((x + y) + z) + w) / 4.
 *   gamma = sqrt(2 ((exx exx + eyy eyy) + ezz ezz) + 4 ((m_0 m_0 + m_1 m_1) + m_2 m_2)), eaa = center_rate[cid + n_center*a].
 * Shear-rate field: one value per cell of the simulation grid (field_n*, the lattice AVS_FIELD_VISCOSITY is given on), x fastest.  From
 *   the level-0 cell the label pyramid is climbed, as avs_sample_velocity does, to the lowest level whose cell over it is ACTIVE; that cell's
 *   centre id cid gives (float)gamma[cid], the fp64 value rounded once.  No ACTIVE cell over it, or a centre index that is no id: 0.
 *   Every entry of `field` is written.
 * Summary (may be NULL; struct_size: IN, the protocol of avs_stress_check -- only that many bytes are written; below offsetof(which) + 4
 *   or above 4096: AVS_EINVAL).  A summary always evaluates all three passes.  empty_*: stencils with cnt == 0 (centres: lists, three per
 *   centre); boundary_*: stencils with bcnt > 0; nonfinite: edge and centre rates that are NaN or Inf.
 *   dissipation_edge = sum_e w_e eps_e^2 and dissipation_center = sum_cells w_c ((exx^2 + eyy^2) + ezz^2), with the integration weights
 *   of the stencils (avs_get_edge_stencils / avs_get_center_stencils: w_e = 4 dt mu V_e, w_c = 2 dt mu V_c, V in fine-voxel units): their
 *   sum is dt / dx^3 times the integral of 2 mu eps:eps over the liquid, u^T (A - M_u) u of the system the solve inverts where no stencil
 *   carries a boundary term.  An edge whose rate is not finite and a cell with a rate that is not finite are left out of the sums; maxima
 *   are over finite values (max_shear_rate over the cells' gamma).  The sums are deterministic: a partial sum per 256 consecutive
 *   stencils, the partial sums folded in a fixed order, no floating atomics -- the same inputs give the same bytes on every call, in
 *   every fresh context and for every grid size.
 * Outputs: any of edge_rate, center_rate, cell_shear_rate and summary may be NULL; only the passes the others need are run.  All four NULL:
 *   AVS_OK, nothing is launched.  n_edge == n_center == 0: AVS_OK, the summary is zero, the field is zero.  AVS_MEM_DEVICE arrays are
 *   written by the kernels directly on the context's stream (the memory rules of avs_get_octree_cells); the call returns once the summary,
 *   if asked for, is on the host.  AVS_MEM_HOST arrays are staged and complete on return.  Scratch (rates, the cell array, partial sums,
 *   the raw summary, staging) stays in the context.
 * State: stencils (avs_build_stencils / avs_assemble) and the vector named by `which`, else AVS_ESTATE; slab-local contexts: AVS_ESTATE.
 *   which not one of the two values, an unknown memory space, a NULL field: AVS_EINVAL. */
enum { AVS_RATES_OF_SOLUTION = 0, AVS_RATES_OF_INITIAL_GUESS = 1 };
enum { AVS_EDGE_LOOKUP_OWN = 0, AVS_EDGE_LOOKUP_CHILD = 1, AVS_EDGE_LOOKUP_GRANDCHILD = 2, AVS_EDGE_LOOKUP_SKIPPED = 3 };
typedef struct avs_strain_summary {
    int32_t struct_size;                 /* IN: sizeof(avs_strain_summary) of the caller's header */
    int32_t which;
    int64_t n_edge, n_center;            /* stencils evaluated: n_edge edge stencils, 3 n_center centre lists */
    int64_t empty_edges, empty_centers;  /* cnt == 0 (lists: 3 per centre) */
    int64_t boundary_edges, boundary_centers; /* bcnt > 0 */
    int64_t nonfinite;                   /* rates that are NaN / Inf */
    int64_t edge_lookups[4];             /* how the cell pass resolved its 12 n_center edge slots (AVS_EDGE_LOOKUP_*) */
    int64_t empty_pairs;                 /* (cell, edge axis) with no contributing edge */
    double dissipation_edge, dissipation_center;
    double max_abs_edge_rate, max_abs_center_rate, max_shear_rate;   /* over finite values */
} avs_strain_summary;
avs_status avs_get_strain_rates(avs_ctx *ctx, int32_t which,
                                double *edge_rate        /* n_edge,      may be NULL */,
                                double *center_rate      /* 3*n_center, list id = cell id + n_center*axis, may be NULL */,
                                double *cell_shear_rate  /* n_center,    may be NULL */,
                                avs_strain_summary *summary /* may be NULL */, avs_memspace where);
avs_status avs_get_shear_rate_field(avs_ctx *ctx, int32_t which, float *field /* field_nx*field_ny*field_nz, x fastest */, avs_memspace where);

/* A shear-dependent viscosity mu(gamma) evaluated on the device from the shear rates above and, if asked for, installed as the context's
 * AVS_FIELD_VISCOSITY without a pass through the caller: provisional fields, avs_build_stencils, avs_build_initial_guess,
 * avs_apply_viscosity_model(AVS_RATES_OF_INITIAL_GUESS, install = 1), avs_assemble, avs_solve -- and for a fixed-point (Picard) loop
 * avs_apply_viscosity_model(AVS_RATES_OF_SOLUTION) after the solve, its max_relative_change the stopping measure.
 * which, the state it needs, the memory-space rules and the struct_size protocol of the summary: those of avs_get_shear_rate_field /
 *   avs_strain_summary.  Slab-local contexts: AVS_ESTATE.
 * Per centre id cid: g = cell_shear_rate[cid], the fp64 value avs_get_strain_rates defines.  All of this step is fp64, one rounding per
 *   operation; pow and expm1 are those of the device's math library.
 *     AVS_VISCOSITY_CARREAU_YASUDA    m = mu_inf + (mu_0 - mu_inf) * pow(1 + pow(lambda * g, a), (n - 1) / a)
 *     AVS_VISCOSITY_HERSCHEL_BULKLEY  m = consistency * pow(g, n - 1) + Y.  tau_y == 0: the term Y is skipped.  Else Y = tau_y * regularisation
 *                                     where g == 0, and Y = (tau_y * (-expm1(-regularisation * g))) / g elsewhere (Papanastasiou).
 *   A NaN m, or a g that is not finite: the id has no value and is counted in nonfinite.  Otherwise m < mu_min: m = mu_min (clamped_low);
 *   m > mu_max: m = mu_max (clamped_high) -- a +inf from pow(0, n - 1) with n < 1 clamps to mu_max.  Then P[cid] = (float)m, one rounding
 *   after the clamp; P > 0 always.
 * Per cell of the simulation grid (field_n*), M, the model's value there:
 *     covered    the climb of avs_get_shear_rate_field finds an ACTIVE cell whose centre index is an id that has a value: M = P of that id;
 *     fringe     not covered, but at least one of the up to 26 neighbours (x, y, z each -1 .. +1) inside the simulation grid is covered:
 *                M = (float)(S / count), S the fp64 sum of (double)P of the covered neighbours, added z slowest, x fastest, count their
 *                number.  A free surface thus continues the liquid's viscosity one cell into the air, where the edge samples of the
 *                assembly reach, instead of mu(0);
 *     untouched  any other cell keeps the viscosity it has.
 *   Relaxation against old, the context's current viscosity at the cell (its field, or its constant): untouched: new = old; relaxation ==
 *   1: new = M; else new = (float)((double)old + relaxation * ((double)M - (double)old)).
 * mu_out (may be NULL) receives new for every cell of the simulation grid.  install != 0: new becomes the context's AVS_FIELD_VISCOSITY
 *   exactly as avs_set_scalar_field(AVS_FIELD_VISCOSITY) with that array would make it -- the border cells replicated onto the padded
 *   lattice, and the same invalidation: stencils, initial guess, system and SOLUTION are gone afterwards (build or assemble again; a
 *   second call, or a strain entry, then reports AVS_ESTATE until they are back).  The kernels write the context's next lattice
 *   directly; no copy of the field is staged.
 * Summary (may be NULL): counts of cells (covered + fringe + untouched = field_nx field_ny field_nz) and of centre ids (clamped_low,
 *   clamped_high, nonfinite, of n_center).  Over covered cells: min_viscosity and max_viscosity of M (0 without a covered cell),
 *   max_shear_rate = the largest g among the ids that give cells their value (ids with a value whose cell starts inside the simulation
 *   grid), max_relative_change = max of fabs((double)new - (double)old) / (double)old in fp64 over the covered cells with old > 0.
 *   Integer counts and maxima only, no floating atomics: the same inputs give the same bytes on every call, in every fresh context and for
 *   every grid size.
 * Parameters: those the kind reads are checked, the others ignored.  Carreau-Yasuda: mu_0, mu_inf, lambda finite and >= 0, a finite and
 *   > 0, n finite.  Herschel-Bulkley: consistency, tau_y, regularisation finite and >= 0, regularisation > 0 where tau_y != 0, n finite.
 *   Both: mu_min finite with (float)mu_min > 0, mu_max finite as a float, mu_min <= mu_max, relaxation in (0, 1], struct_size =
 *   sizeof(avs_viscosity_model).  A violation (a NaN is one): AVS_EINVAL, the message names the parameter.  An unknown which / memory
 *   space / kind, a NULL model: AVS_EINVAL.  mu_out == NULL, install == 0 and summary == NULL: AVS_OK, nothing is launched.
 * AVS_MEM_DEVICE mu_out is written by the kernels on the context's stream; AVS_MEM_HOST is staged and complete on return; the call returns
 *   once the summary, if asked for, is on the host.  Scratch (the per-id array, the painted array, staging, the lattice the next install
 *   fills) stays in the context. */
enum { AVS_VISCOSITY_CARREAU_YASUDA = 0, AVS_VISCOSITY_HERSCHEL_BULKLEY = 1 };
typedef struct avs_viscosity_model {
    int32_t struct_size, kind;                 /* sizeof(avs_viscosity_model), AVS_VISCOSITY_* */
    double mu_0, mu_inf, lambda, a, n;         /* Carreau-Yasuda */
    double consistency, tau_y, regularisation; /* Herschel-Bulkley (n shared); Papanastasiou m */
    double mu_min, mu_max;                     /* clamp; (float)mu_min > 0, mu_min <= mu_max, both finite */
    double relaxation;                         /* omega in (0, 1] */
} avs_viscosity_model;
typedef struct avs_viscosity_summary {
    int32_t struct_size;                 /* IN: sizeof(avs_viscosity_summary) of the caller's header */
    int32_t which;
    int32_t kind, installed;             /* the model's kind; 1 = the result is the context's viscosity field now */
    int64_t n_center;                    /* centre ids evaluated */
    int64_t covered, fringe, untouched;  /* cells of the simulation grid */
    int64_t clamped_low, clamped_high, nonfinite; /* centre ids */
    double min_viscosity, max_viscosity, max_shear_rate, max_relative_change; /* over covered cells */
} avs_viscosity_summary;
avs_status avs_apply_viscosity_model(avs_ctx *ctx, int32_t which, const avs_viscosity_model *model,
                                     float *mu_out /* field_nx*field_ny*field_nz, x fastest; may be NULL */,
                                     int32_t install, avs_viscosity_summary *summary /* may be NULL */, avs_memspace where);

/* ------------------------------------------------------------------------------------------
 * Seam A: only the solve (replaces cpp:611-643).  CSR with int32 row pointers/columns, fp64
 * values; x_inout holds the initial guess on entry and the solution on return.
 * ---------------------------------------------------------------------------------------- */
avs_status avs_pcg_csr(int64_t n, const int32_t *row_ptr, const int32_t *col, const double *val,
                       const double *b, double *x_inout, double tolerance, int32_t max_iterations,
                       avs_memspace where, int32_t device, void *stream, avs_solve_info *info);

/* Is this CSR system one avs_pcg_csr is defined for?  avs_pcg_csr hands row_ptr, col and val to its kernels unread: a column outside
 * [0, n) or a row pointer that runs backwards is an out-of-bounds gather there, and a missing or non-positive diagonal, a NaN or an
 * unsymmetric matrix is a solve that does not converge without saying why.  avs_check_csr evaluates eight rules on the device and reports
 * a 64-bit count per rule, the first violating position and a few measurements.  Nothing else in the library calls it, it writes nothing
 * the caller owns, and every other entry behaves as without it.  avs_check_system is the same check on the system a context assembled.
 * n rows, row_ptr has n + 1 entries; nnz is the caller's statement of how long col and val are: entry nnz and anything beyond it is never
 * read, whatever row_ptr says.  Every rule is evaluated independently, entry by entry; a position counts at most once per rule:
 *   0 ROW_PTR   (always) index i in 0 .. n: row_ptr[i] < 0 or > nnz; i == 0 and row_ptr[0] != 0; i == n and row_ptr[n] != nnz; i < n and
 *               row_ptr[i] > row_ptr[i + 1].  If rule 0 is violated nothing else is evaluated (the other rules walk rows through
 *               row_ptr): evaluated = 1, every other count and every measurement is 0, first_row = first_col = -1.
 *   1 COLUMN    (always, once rule 0 holds) entry k: col[k] < 0 or >= n.  Such entries are skipped by rules 5 .. 7; no value read from
 *               the caller's arrays is used as an address without this test.
 *   2 VALUE     (AVS_CSR_CHECK_VALUES) entry k: val[k] is NaN or +-Inf.
 *   3 VECTOR    (AVS_CSR_CHECK_VALUES, and only if b or x is given) row i: b[i] or x[i] is NaN or +-Inf.
 *   4 ORDER     (AVS_CSR_CHECK_ORDER) entry k that is not the first of its row: col[k] <= col[k - 1] -- rows strictly ascending, hence no
 *               repeated column, as Eigen's compressed matrix (cpp:613-614) and the device triplet merge hold them.  The SpMV forms
 *               accept unordered rows: a caller who knows its rows are unordered leaves this bit out.
 *   5 DIAGONAL  (AVS_CSR_CHECK_DIAGONAL) row i: no entry with col == i, or the last such entry (the one the Jacobi preconditioner reads)
 *               is not > 0 (NaN is not > 0).
 *   6 PATTERN   (AVS_CSR_CHECK_SYMMETRY) entry k = (i, j) with j in range and j != i: row j has no entry with column i.
 *   7 SYMMETRY  (AVS_CSR_CHECK_SYMMETRY) entry k = (i, j) as in rule 6 whose partner p -- the first entry of row j with column i -- exists:
 *               val[k] and val[p] are finite and |val[k] - val[p]| > symmetry_tolerance (absolute, the caller's number, typically a
 *               multiple of max_abs_value; one subtraction and one comparison).
 * Measurements (rule 0 holding): empty_rows, longest_row (entries); with AVS_CSR_CHECK_SYMMETRY, else 0: max_abs_value = the largest
 *   |val[k]| over the finite entries, and over the pairs (k, p) of rule 7 with both values finite asymmetric_entries = pairs with
 *   val[k] != val[p] and max_abs_asymmetry = the largest |val[k] - val[p]|.
 * what: any of the AVS_CSR_CHECK_* bits; 0 runs rules 0 and 1 only; any other bit: AVS_EINVAL.  A rule that was not asked for reports 0
 *   and is not launched.  evaluated: bit r = rule r was evaluated.  n == 0: rule 0 on the single pointer, nothing else (evaluated = 1).
 * first_*: the violating position that comes first by (rule, index); first_rule = first_index = first_row = first_col = -1 when passed.
 *   first_index: the row_ptr index (rule 0), the entry k (rules 1, 2, 4, 6, 7), the row i (rules 3, 5).  first_row: the row that owns
 *   entry k, or the row i (-1 for rule 0); first_col: col[k] as stored, even out of range (-1 for rules 0, 3, 5).
 * Arguments: n, nnz in [0, 2^31); row_ptr non-NULL; col and val non-NULL when nnz > 0; b, x may be NULL (n entries each otherwise);
 *   symmetry_tolerance finite and >= 0; device in range; report non-NULL with struct_size set (IN, as in avs_matrix_format: only that
 *   many bytes are written).  Anything else: AVS_EINVAL with a message in avs_last_error.
 * AVS_MEM_DEVICE arrays are read in place on `stream` (NULL: a stream of the library's own), AVS_MEM_HOST arrays are staged; the call
 *   returns once the report is on the host (one more wait after the row_ptr pass: rule 0 decides whether the rest may run).
 * avs_check_system: the context's reference-numbered row_ptr, col, val and rhs (what avs_get_csr hands out) as b, and the initial guess
 *   as x.  Needs avs_assemble (AVS_ESTATE otherwise, and after avs_dist_assemble: no global matrix exists); scratch (the raw report, one
 *   byte per row) stays in the context; nothing a later avs_solve reads is changed.
 * The same arrays give the same report on every call.  The partner search of rules 6 / 7 is a binary search in rows that are strictly
 *   ascending and a linear scan (row length probes per entry) in rows that are not. */
enum { AVS_CSR_CHECK_VALUES = 1, AVS_CSR_CHECK_ORDER = 2, AVS_CSR_CHECK_DIAGONAL = 4, AVS_CSR_CHECK_SYMMETRY = 8,
       AVS_CSR_CHECK_ALL = 15 };
enum { AVS_CSR_RULE_ROW_PTR = 0, AVS_CSR_RULE_COLUMN = 1, AVS_CSR_RULE_VALUE = 2, AVS_CSR_RULE_VECTOR = 3,
       AVS_CSR_RULE_ORDER = 4, AVS_CSR_RULE_DIAGONAL = 5, AVS_CSR_RULE_PATTERN = 6, AVS_CSR_RULE_SYMMETRY = 7,
       AVS_CSR_RULES = 8 };
typedef struct avs_csr_check {
    int32_t struct_size;          /* IN: sizeof(avs_csr_check) of the caller's header */
    int32_t passed;               /* 1 = no evaluated rule is violated */
    int32_t evaluated;            /* bit r: rule r was evaluated */
    int32_t first_rule;           /* -1 when passed */
    int64_t first_index;          /* position in the rule's array: row_ptr index (rule 0), entry k (1, 2, 4, 6, 7), row i (3, 5) */
    int32_t first_row, first_col; /* row owning the entry / the stored column (as stored, even out of range); -1 where not applicable */
    int64_t violations[AVS_CSR_RULES];
    int64_t empty_rows, longest_row;
    int64_t asymmetric_entries;   /* measurements of the SYMMETRY bit; 0 when not asked */
    double max_abs_value, max_abs_asymmetry;
} avs_csr_check;
avs_status avs_check_csr(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val,
                         const double *b /* may be NULL */, const double *x /* may be NULL */,
                         uint32_t what, double symmetry_tolerance, avs_memspace where, int32_t device, void *stream,
                         avs_csr_check *report);
avs_status avs_check_system(avs_ctx *ctx, uint32_t what, double symmetry_tolerance, avs_csr_check *report);

/* Did x solve A x = b?  The true residual r = b - A x in fp64, from the plain CSR: the output half of the checks above.  avs_solve_info.error
 * is the recurrence's own sqrt(|r|^2 / |b|^2), the updated residual of whichever loop and storage form ran; this is the product itself.
 * Nothing else in the library calls either entry, and every other entry behaves as without them.
 * Rows (fp64, one rounding per operation): y_i = 0; for k = row_ptr[i] .. row_ptr[i + 1] - 1 in stored order: y_i = y_i + val[k] * x[col[k]];
 *   r_i = b_i - y_i.  The order of the stream SpMV and of a plain CSR loop, so r is defined bit for bit (the sign and payload of a NaN aside).  Rows may
 *   be unordered and may repeat columns; an empty row gives r_i = b_i.  AVS_PRECISION_F32 contexts are evaluated the same way on the float
 *   values their fp64 arrays hold.  residual, if given, receives every r_i (n entries), non-finite ones included.
 * Counters: nonfinite_x, nonfinite_b: entries that are NaN or +-Inf; nonfinite_residual: rows whose r_i is.  rows_summed: rows with x_i,
 *   b_i and r_i all finite.  Every sum and every maximum below runs over those rows only:
 *   rhs_norm2 = sum b_i b_i, residual_norm2 = sum r_i r_i, x_dot_ax = sum x_i y_i, x_dot_b = sum x_i b_i (the energy 0.5 xAx - xb is the
 *   caller's subtraction), max_abs_x = max |x_i|, max_abs_residual = max |r_i| and max_residual_row the smallest row that attains it (-1
 *   if rows_summed == 0); over the rows among them whose x0_i is finite too: update_norm2 = sum (x_i - x0_i)^2, max_abs_update = max
 *   |x_i - x0_i| (both 0 when no x0 is known).  A sum is one partial sum per 256 consecutive rows, folded in a fixed order: the same
 *   arrays give the same bytes on every call, in every context, for every grid.
 * relative_residual = sqrt(residual_norm2 / rhs_norm2), Eigen's error() (cpp:630); with rhs_norm2 == 0: 0 if residual_norm2 == 0, else +Inf.
 * avs_check_solution: the context's reference-numbered row_ptr, col, val and rhs, read in place (the arrays avs_check_system reads).
 *   which = AVS_CHECK_OF_SOLUTION: x is the solution (avs_solve, avs_set_solution) and x0 the initial guess;
 *   AVS_CHECK_OF_INITIAL_GUESS: x is the initial guess (the update is 0).  AVS_ESTATE without a system (and after avs_dist_assemble or on
 *   a slab-local context: no global matrix exists) or without the named vector.  claimed_*: avs_solve_info of the last avs_solve, while
 *   x is still what that solve left and the matrix the one it solved (avs_set_solution, a gathered partitioned solution and a
 *   re-assembly drop the claim); else -1 / NaN.  Scratch stays in the context; nothing a later avs_solve reads is changed.
 * avs_check_csr_solution (seam A): arguments and memory rules of avs_check_csr; b and x non-NULL when n > 0, x0 and residual may be NULL.
 *   col is an address here, so rules 0 and 1 of avs_check_csr run first on the same stream: if either is violated the call returns
 *   AVS_OK with evaluated = 0, every other figure 0 and residual untouched.  claimed_* = -1 / NaN.  n == 0: evaluated = 1, all 0.
 * report may be NULL if residual is given (avs_check_csr_solution: report non-NULL); struct_size is IN (only that many bytes are written).
 *   Unknown which / memory space, both outputs NULL, struct_size out of range: AVS_EINVAL with a message. */
enum { AVS_CHECK_OF_SOLUTION = 0, AVS_CHECK_OF_INITIAL_GUESS = 1 };   /* same values as AVS_RATES_OF_* */
typedef struct avs_solution_check {
    int32_t struct_size;          /* IN: sizeof(avs_solution_check) of the caller's header */
    int32_t which;
    int32_t evaluated;            /* 1 = rows were walked; 0 = seam A only: rule 0 or 1 of avs_check_csr is violated, all else 0 */
    int32_t claimed_converged;    /* avs_solve_info.converged of the solve that left x, else -1 */
    int32_t claimed_iterations;   /* likewise, else -1 */
    int32_t reserved;
    int64_t n, nnz;
    int64_t nonfinite_x, nonfinite_b, nonfinite_residual;
    int64_t rows_summed;
    double rhs_norm2, residual_norm2, relative_residual;
    double max_abs_residual;
    int64_t max_residual_row;
    double max_abs_x;
    double x_dot_ax, x_dot_b;
    double update_norm2, max_abs_update;
    double claimed_error;         /* avs_solve_info.error of that solve, else NaN */
} avs_solution_check;
avs_status avs_check_solution(avs_ctx *ctx, int32_t which, double *residual /* n, may be NULL */,
                              avs_solution_check *report /* may be NULL if residual is given */, avs_memspace where);
avs_status avs_check_csr_solution(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val,
                                  const double *b, const double *x, const double *x0 /* may be NULL */,
                                  double *residual /* may be NULL */, avs_memspace where, int32_t device, void *stream,
                                  avs_solution_check *report);

/* Why does a solve take the iterations it takes?  m steps of the symmetric Lanczos recurrence on the operator the solve inverts, S A S with
 * S = diag(s): op = AVS_SPECTRUM_OF_JACOBI: s_i = 1 / sqrt(d_i), the Jacobi-scaled matrix D^-1/2 A D^-1/2; AVS_SPECTRUM_OF_MATRIX: s_i = 1,
 * A itself (AVS_PRECONDITIONER_NONE).  The result is the Ritz values, error bounds of the two extreme ones, a Gershgorin bound of
 * lambda_max, a condition estimate and the classical CG iteration bound; a Ritz value <= 0 certifies that the matrix is not positive
 * definite.  The product is the fp64 stream product of avs_check_solution over the plain reference-numbered CSR, whichever storage form
 * and loop a solve would use.  Nothing else in the library calls either entry, and every other entry behaves as without them.
 * Everything is fp64 with one rounding per operation; the matrix is taken as symmetric (avs_check_csr, rule 7, says whether it is).
 * Diagonal and scale: d_i is the LAST entry of row i with col == i (what the Jacobi preconditioner and rule 5 of avs_check_csr read);
 *   s_i = 1.0 / sqrt(d_i).  A row without a diagonal entry, or whose d_i is not > 0 or not finite, counts in bad_diagonal and has s_i = 0;
 *   with bad_diagonal > 0 nothing else is evaluated (evaluated = 0, AVS_OK).  OF_MATRIX never looks at the diagonal (bad_diagonal = 0).
 * gershgorin_max = max_i g_i with g_i = 0; g_i = g_i + |val[k]| * (s_i * s_col[k]) for the entries of row i in stored order: an upper
 *   bound of lambda_max up to its own rounding (it is NOT rounded outward).  The maximum is taken over bit patterns of non-negative
 *   doubles, so it does not depend on any order; a row sum that is not finite gives +Inf.
 * Start vector v: AVS_SPECTRUM_START_RESIDUAL: v = s o (b - A x0), rows formed as in avs_check_solution -- the Krylov space CG itself
 *   works in; AVS_SPECTRUM_START_HASH: v_i = (double)(splitmix64(i) >> 11) * 2^-53 - 0.5, exact arithmetic, so the vector is defined
 *   bit for bit (splitmix64(i): z = i + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 *   0x94D049BB133111EB; z ^ (z >> 31), in 64-bit unsigned arithmetic); AVS_SPECTRUM_START_VECTOR: the caller's array.  beta[0] =
 *   start_norm = sqrt(sum v_i v_i); v_0 = v / beta[0], divided element by element.  A start norm that is zero or not finite gives
 *   steps_taken = 0 (nonfinite = 1 if it was not finite).
 * Step j = 0 .. steps - 1 (Paige's ordering): u = s o v_j; y_i = sum val[k] * u[col[k]], left to right in stored order; t_i = s_i * y_i
 *   - beta[j] * v_{j-1,i} (no beta term at j = 0); alpha[j] = sum v_{j,i} t_i; w_i = t_i - alpha[j] * v_{j,i}; beta[j + 1] = sqrt(sum
 *   w_i w_i); v_{j+1} = w / beta[j + 1], by division.  The effective number of steps is min(steps, n).  No reorthogonalisation.
 * Stop before v_{j+1} is formed, with steps_taken = j + 1: alpha[j] or beta[j + 1] is not finite (nonfinite = 1); or not (beta[j + 1] >
 *   2^-36 * (|alpha[j]| + beta[j])) (breakdown = 1: the Krylov space is invariant to working accuracy and the Ritz values are
 *   eigenvalues).  The threshold lies some ten bits below the square root of the unit roundoff: sum v^2 is not exactly 1, so an exact
 *   zero almost never occurs, and a w that small is rounding error of t and alpha v, not a new direction.
 * Sums: every sum is one partial sum per 256 consecutive rows, folded in a fixed order, without floating-point atomics: the same arrays
 *   give the same bytes on every call, in every context, for every grid.
 * Host part, k = steps_taken: T_k = tridiag(beta[1 .. k - 1]; alpha[0 .. k - 1]); ritz = its eigenvalues in ascending order (implicit QL);
 *   lambda_min, lambda_max the extreme ones; lambda_*_bound = beta[k] * |last component of that Ritz vector|: an eigenvalue of the
 *   operator lies within that distance of the Ritz value.  indefinite = 1 if lambda_min <= 0.  condition_estimate = lambda_max /
 *   lambda_min (+Inf if indefinite): a LOWER bound of the condition number, since the Ritz values lie inside the spectrum (lambda_min
 *   converges from above).  iteration_bound = ceil(0.5 sqrt(condition_estimate) ln(2 / tolerance)) for tolerance in (0, 1) and a finite
 *   estimate, else -1: the bound of the A-norm of the error, not Eigen's residual rule (avs_solve_info.error).  With steps_taken = 0:
 *   all of these 0 and iteration_bound -1; if a step left a non-finite alpha or beta: NaN and -1.  Without reorthogonalisation the
 *   extremes are reliable, multiplicities are not (converged Ritz values come back as copies).
 * Outputs: alpha (steps), beta (steps + 1) and ritz (steps) are always HOST arrays and complete on return (0 behind what the steps taken
 *   wrote); scale (n) and basis (n x (steps + 1), column-major, column j = v_j) follow `where`; every one may be NULL.  scale is written
 *   whenever the diagonal was read (also with bad_diagonal > 0).  basis holds columns 0 .. steps_taken - 1, and column steps_taken unless
 *   the recurrence stopped; what lies behind them is unspecified.  n == 0: evaluated = 1, steps_taken = 0.
 * Scratch: five n-vectors of doubles (s, u, v_{j-1}, v_j, w), kept in the context: 300 MB at 512^3.  Nothing a later avs_assemble,
 *   avs_solve or transfer reads is changed.  The recurrence is enqueued whole; the stop decision is a word in device memory.
 * avs_estimate_spectrum: the context's reference-numbered row_ptr, col, val, rhs and initial guess, read in place.  AVS_ESTATE where
 *   avs_check_solution(AVS_CHECK_OF_INITIAL_GUESS) returns it; AVS_SPECTRUM_START_VECTOR: AVS_EINVAL.
 * avs_estimate_csr_spectrum (seam A): arguments and memory rules of avs_check_csr_solution; b and x0 non-NULL for START_RESIDUAL,
 *   start_vector for START_VECTOR (n > 0), otherwise they may be NULL.  Rules 0 and 1 of avs_check_csr run first on the same stream: if
 *   either is violated the call returns AVS_OK with evaluated = 0, every figure 0 and no array but alpha, beta and ritz (zeros) written.
 * steps outside [1, AVS_SPECTRUM_MAX_STEPS], unknown op / start / memory space, report NULL or its struct_size out of range, n or nnz
 *   outside [0, 2^31): AVS_EINVAL with a message.  struct_size is IN (only that many bytes are written). */
enum { AVS_SPECTRUM_OF_JACOBI = 0, AVS_SPECTRUM_OF_MATRIX = 1 };              /* s_i = 1/sqrt(d_i)  |  s_i = 1 */
enum { AVS_SPECTRUM_START_RESIDUAL = 0, AVS_SPECTRUM_START_HASH = 1, AVS_SPECTRUM_START_VECTOR = 2 };
#define AVS_SPECTRUM_MAX_STEPS 512
typedef struct avs_spectrum {
    int32_t struct_size;          /* IN: sizeof(avs_spectrum) of the caller's header */
    int32_t evaluated;            /* 1 = the recurrence was set up; 0 = rule 0 or 1 of avs_check_csr violated (seam A), or bad_diagonal > 0 */
    int32_t op, start, steps_asked;
    int32_t steps_taken;          /* k: alpha[0 .. k - 1] and beta[0 .. k] are the recurrence's */
    int32_t breakdown, nonfinite, indefinite;
    int64_t n, nnz;
    int64_t bad_diagonal;
    double start_norm;
    double lambda_min, lambda_max, lambda_min_bound, lambda_max_bound;
    double gershgorin_max;
    double condition_estimate;
    double tolerance;             /* as given */
    int64_t iteration_bound;
} avs_spectrum;
avs_status avs_estimate_spectrum(avs_ctx *ctx, int32_t op, int32_t start, int32_t steps, double tolerance,
                                 double *alpha /* steps */, double *beta /* steps + 1 */, double *ritz /* steps */, double *scale /* n */,
                                 double *basis /* n x (steps + 1), column j = v_j, column-major */, avs_memspace where,
                                 avs_spectrum *report);
avs_status avs_estimate_csr_spectrum(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val,
                                     const double *b, const double *x0, const double *start_vector, int32_t op, int32_t start,
                                     int32_t steps, double tolerance, double *alpha, double *beta, double *ritz, double *scale,
                                     double *basis, avs_memspace where, int32_t device, void *stream, avs_spectrum *report);

/* (measurement / test entries -- single SpMV launches, kernel sweeps, stream probes -- live in include/avs_probe.h and libavs_probe.so) */

/* ------------------------------------------------------------------------------------------
 * Pre-pass on the device (SURVEY 8(f) "next #1/#4"): what solveGasSubclass computes BEFORE the hot
 * path -- integration weights (cpp:712-766), refinement mask (cpp:815-867), octree label pyramid
 * (HDK_OctreeGrid.cpp:4-243), classification (cpp:1087-1443) and serial numbering in HDK tile
 * order (cpp:1445-1715) -- from the liquid / solid SDFs (centre lattice, fp32, x fastest).
 * ---------------------------------------------------------------------------------------- */
typedef struct avs_prepass avs_prepass;
typedef struct {
    int32_t nx, ny, nz;         /* powers of two */
    double dx;
    int32_t desired_levels;     /* getOctreeLevels(), cpp:263 */
    int32_t n_super;            /* getNumberSuperSamples(), cpp:756 (default 3) */
    double extrapolation_scale; /* getExtrapolation(), cpp:243 (default 0.5) */
    int32_t device;
    void *stream;
    /* Resolution of the SIMULATION grid the SDFs are given on when it is not a power of two per axis: nx, ny, nz are then the
     * octree grid HDK_OctreeGrid::init stretches it to (smallest powers of two that contain it, oct.cpp:10-24), cells outside
     * the simulation grid stay INACTIVE (oct.cpp:375-379).  0 = nx, ny, nz.  The SDFs are read with clamped coordinates outside
     * their grid (SIM_RawField border behaviour); the liquid must not touch the border of the simulation grid.  All getters
     * below return arrays on the (padded) octree lattices. */
    int32_t field_nx, field_ny, field_nz;
} avs_prepass_desc;
typedef struct {
    int32_t levels;                       /* after capping, HDK_OctreeGrid.cpp:198-211; 0 = no liquid */
    int64_t n_velocity, n_edge, n_center; /* cpp:395-408 */
    int64_t n_regular;                    /* regularVelocityDOFcount, cpp:323 */
    double weights_ms, octree_ms, classify_ms, number_ms;
} avs_prepass_info;
avs_status avs_prepass_create(const avs_prepass_desc *desc, avs_prepass **out);
/* Options of the pre-pass; they take effect at the next avs_prepass_run.  FINE_BANDWIDTH belongs to the refinement mask (cpp:815-867),
 * APPLY_SOLID_WEIGHTS to the integration weights (cpp:768-790).
 *   AVS_PREPASS_OPTION_FINE_BANDWIDTH  the reference's "Fine Layer Bandwidth": cells within inner = dx * max(2, value) INSIDE the liquid
 *     surface stay fine (SYSmax(2., fpreal(getFineBandwidth())), cpp:259-261); inner also enters the solid rule, solid > -inner -
 *     extrapolation (cpp:853).  Default 2, and anything <= 2 behaves as 2 -- which is all the reference's own build ever gets: its getter
 *     does not match the UI token.  The outer band stays 3 dx.  A non-finite value or an unknown option: AVS_EINVAL, nothing
 *     changes.
 *   AVS_PREPASS_OPTION_APPLY_SOLID_WEIGHTS  the reference's "Apply Solid Weights" (UI token applySolidWeights, getter
 *     doApplySolidWeights, cpp:60, 244, 768-790: "theta value for applying ghost fluid collision velocities").  0 (default): off;
 *     1: on; any other value, NaN included: AVS_EINVAL, nothing changes.  With the option on AND a solid SDF given to avs_prepass_run the
 *     centre and the three edge weight lattices are divided by the super-sampled fraction of open space; the face weights are never
 *     touched (the reference's faceWeights is an input field that does not see this step).  The rule (HDK's arithmetic is closed source;
 *     this is the project's definition, all fp32, one rounding per operation):
 *       ext32 = (float)(dx * extrapolation_scale), the product in double;  g = solid + ext32 per cell of the lattice the SDFs are given
 *       on (solid > 0 inside the solid: g < 0 is outside the solid grown by the extrapolation), read with clamped coordinates as the
 *       liquid is;  l / S = the number of the n^3 sub-samples whose trilinear interpolation of the liquid / of g is < 0 (same constants,
 *       same lerp order);  w = (float)l / n^3, W = (float)S / n^3;  w' = 0 if l == 0 or S == 0, else w / W (an IEEE fp32 division).
 *     S == n^3 leaves w bit for bit; w' may exceed 1 (up to n^3); w' > 0 implies w > 0, so everything downstream (tile occupancy,
 *     classification, numbering, assembly) runs unchanged on the new values.  avs_prepass_get_weights returns and avs_prepass_apply
 *     lends the scaled lattices.  Without a solid SDF, or with the option off, every lattice is byte for byte what it is without the
 *     option.  Two HDK behaviours are NOT pinned by the reference tree and assumed here: how computeSDFWeightsSampled
 *     applies its dilate argument (here: the shift of the cell values above, never a non-zero threshold on interpolated values --
 *     rounding inside the lerps would break the exact sign shortcuts), and what setScaleDivideThreshold does where the divisor is 0
 *     (here: the result is 0). */
typedef enum { AVS_PREPASS_OPTION_FINE_BANDWIDTH = 0, AVS_PREPASS_OPTION_APPLY_SOLID_WEIGHTS = 1 } avs_prepass_option;
avs_status avs_prepass_set_option(avs_prepass *pp, avs_prepass_option option, double value);
/* What the weights pass of the last avs_prepass_run did with the solid SDF (struct_size: IN, only that many bytes are written; callable
 * before any run: everything but enabled is 0 then).  Per lattice, [4] = centre, edge x, edge y, edge z: modified = samples with
 * w' != w, zeroed = samples with l > 0 and S == 0, above_one = samples with w' > 1, max_weight = the largest w'.  All zero when
 * applied == 0.  The counts are integer atomics and the maximum is taken on the bit pattern: the same inputs give the same numbers in
 * every call and every fresh object, whatever earlier runs left in the lattices (a brick that is not stored again still counts what it
 * holds).  near_bricks: the 32x4x4 bricks of samples the near kernel computed (any run).  Slab-local mode: the numbers cover the
 * bricks of the rank's window (whole bricks, so the windows of two ranks overlap): they are not meant to be summed over ranks. */
typedef struct {
    int32_t struct_size;   /* IN: sizeof(avs_solid_weights_info) of the caller's header */
    int32_t enabled;       /* the option as set now */
    int32_t applied;       /* 1: the last run had the option on AND a solid SDF */
    float extrapolation;   /* ext32 of the last applied run */
    int64_t modified[4], zeroed[4], above_one[4];
    float max_weight[4];
    int64_t near_bricks;
} avs_solid_weights_info;
avs_status avs_prepass_get_solid_weights_info(avs_prepass *pp, avs_solid_weights_info *info);
/* Indicator-driven refinement: keep the octree fine where a field the host paints says so -- a shear band, a steep viscosity gradient
 * deep inside the liquid, which the surface rule coarsens as far as the grading allows.
 *   indicator: centre lattice of the SIMULATION grid (field_nx x field_ny x field_nz, x fastest) -- the lattice of the SDFs given to
 *     avs_prepass_run and of avs_get_shear_rate_field.  NULL = no refinement (the default); the other arguments are then ignored.
 *   A SEED is a cell with indicator > threshold (a float compare: NaN never marks, +inf does).  The FLAGS are all simulation-grid cells
 *   within Chebyshev (box) distance dilate_cells (0 .. 16) of a seed; cells of the padded octree lattice outside the simulation grid are
 *   never flagged.  The call computes the flags at once, over the whole lattice (slab-local mode included: a rank's window reads them), on
 *   the pre-pass's stream, and returns when they are there; the pre-pass keeps them -- one bit per cell, allocated by the first call --
 *   not the caller's array, for every following run until they are replaced or cleared.
 *   Mask rule of avs_prepass_run: a DEEP cell (sdf <= -inner), which gets mask 0 if the solid rule passes and -1 (coarsen) otherwise, gets
 *   mask 0 if the solid rule passes OR the cell is flagged.  A flag anywhere else has no effect; octree passes, grading, level cap,
 *   classification and numbering are what they are without flags.
 *   dilate_cells outside 0 .. 16 or an unknown memory space: AVS_EINVAL, nothing changes and nothing is launched.
 * avs_prepass_get_refinement: the flags as 0 / 1 on the OCTREE centre lattice (nx * ny * nz, the lattice of avs_prepass_get_mask); all
 *   zero before the first set call and after a clearing one.
 * avs_refinement_info (struct_size: IN, only that many bytes are written): seeds and flagged are the counts of the set call (0 when
 *   cleared); refined is the number of cells of the last avs_prepass_run whose mask the flags changed from -1 to 0 (slab-local mode: inside
 *   the rank's window); set_ms the HIP-event time of the set call's kernels (a host indicator's upload not included). */
avs_status avs_prepass_set_refinement(avs_prepass *pp, const float *indicator, float threshold, int32_t dilate_cells, avs_memspace where);
avs_status avs_prepass_get_refinement(avs_prepass *pp, int8_t *flags /* octree centre lattice nx*ny*nz, 0 / 1 */, avs_memspace where);
typedef struct {
    int32_t struct_size;  /* IN: sizeof(avs_refinement_info) of the caller's header */
    int32_t dilate_cells;
    float threshold;
    int32_t active;       /* 1: flags are set */
    int64_t seeds, flagged, refined;
    double set_ms;
} avs_refinement_info;
avs_status avs_prepass_get_refinement_info(avs_prepass *pp, avs_refinement_info *info);
/* Slab-local pre-pass (round 6; SURVEY 8(e): "each GPU assembles the rows it owns from its slab of the pyramids plus a halo").  The
 * reference's loops are row-local (classification / numbering cpp:1087-1715, octree oct.cpp:395-565), so a rank of a partitioned solve
 * needs them on its slab only.  cuts[0 .. world]: fine-cell coordinates along cut_axis, cuts[0] = 0, cuts[world] = the axis' extent,
 * ascending; rank r owns the faces whose position lies in [cuts[r], cuts[r + 1]).  avs_prepass_run then computes weights, mask, labels,
 * classification and ids only inside the rank's WINDOW: at level l the slab +- 12 level-l cells, rounded out to whole 16-entry tiles
 * (labels on as much more as the coarser levels' windows depend on).  The ids are the reference's GLOBAL ids (cpp:1566-1593 numbers tile
 * after tile through the whole lattice): every tile is counted by the rank that owns its first plane, `allreduce` sums the per-tile counts
 * of all ranks (ONE call per run, a few MB of int32 on the device, in place, enqueued on / synchronised with `stream`), and every rank scans
 * the same array.  The levels cap (oct.cpp:198-211) rides in the same buffer.  Everything inside the window is bit-identical to the
 * single-rank pre-pass; lattice entries outside it are unspecified.  world == 1 or cuts == NULL switches the mode off. */
typedef avs_status (*avs_allreduce_i32_fn)(int32_t *device_data, int64_t count, void *stream, void *user);
avs_status avs_prepass_set_slab(avs_prepass *pp, int32_t cut_axis, const int32_t *cuts, int32_t world_size, int32_t rank,
                                avs_allreduce_i32_fn allreduce, void *user);
/* the window of the last run along the cut axis: entries [lo[l], hi[l]) of the level-l lattices (hi == the level's cell count: to the end) */
avs_status avs_prepass_get_window(avs_prepass *pp, int32_t *lo, int32_t *hi /* AVS_MAX_LEVELS each */, int64_t *n_window /* 3: velocity, edge, centre DOFs inside it */);
void avs_prepass_destroy(avs_prepass *pp);
/* (AVS_MEM_DEVICE arrays on a power-of-two grid are read in place while the call runs -- no copy; host arrays and padded grids are staged) */
avs_status avs_prepass_run(avs_prepass *pp, const float *liquid_sdf, const float *solid_sdf /* NULL: none */, avs_memspace where);
avs_status avs_prepass_get_info(avs_prepass *pp, avs_prepass_info *info);
avs_status avs_prepass_get_labels(avs_prepass *pp, int32_t level, int8_t *out, avs_memspace where);
avs_status avs_prepass_get_mask(avs_prepass *pp, int8_t *out, avs_memspace where);
avs_status avs_prepass_get_index(avs_prepass *pp, avs_index_kind kind, int32_t level, int32_t axis, int32_t *out, avs_memspace where);
/* regularVelocityIndices[axis] (cpp:1445-1512) */
avs_status avs_prepass_get_regular_index(avs_prepass *pp, int32_t axis, int32_t *out, avs_memspace where);
avs_status avs_prepass_get_weights(avs_prepass *pp, avs_field_kind kind /* CENTER / EDGE / FACE weights */, int32_t axis, float *out,
                                   avs_memspace where);
/* the ACTIVE cells of the label pyramid of the last run as points: avs_get_octree_cells (above) on the pre-pass object -- same order,
 * values, capacity protocol and memory rules; enqueued on the pre-pass's stream.  No solve context is needed ("Only Output Octree"). */
avs_status avs_prepass_get_octree_cells(avs_prepass *pp, const double *origin /* 3, NULL = 0,0,0 */, int64_t capacity,
                                        float *position, float *pscale, int32_t *level, int32_t *ijk /* may be NULL */,
                                        int64_t *n_cells, int64_t *per_level /* AVS_MAX_LEVELS, may be NULL */, avs_memspace where);
/* the invariants of the pyramids of the last run: avs_check_octree (above) on the pre-pass object -- same rules, report and state errors;
 * enqueued on the pre-pass's stream */
avs_status avs_prepass_check_octree(avs_prepass *pp, uint32_t what, avs_octree_check *report);
/* the invariants of the edge and centre stress index pyramids of the last run: avs_check_stress_indices (above) on the pre-pass object */
avs_status avs_prepass_check_stress_indices(avs_prepass *pp, uint32_t what, avs_stress_check *report);
/* hands labels, index pyramids, DOF counts, regular-grid indices and the three weight fields to a solve context created with
 * levels == info.levels on the same device.  BY REFERENCE (round 5; it used to copy ~12 full-size lattices per level set: 78 GB at
 * 1024^3): the context holds the pre-pass's allocations; the pre-pass keeps two per lattice and its next avs_prepass_run fills the set no
 * context references, so what a context was given stays as it is until its next avs_prepass_apply, and avs_prepass_destroy may be called
 * while contexts still use what they were lent.  An avs_set_* call on the context replaces a lent lattice by the context's own copy.
 * Frame after frame on one avs_prepass object the run also skips what its allocations already hold from their last filling (weight
 * bricks far from the surface whose constant has not changed, index tiles outside the last occupancy): outputs identical to a fresh
 * object's, bit for bit; AVS_PREPASS_TEMPORAL=0 in the environment at avs_prepass_create switches it off. */
avs_status avs_prepass_apply(avs_prepass *pp, avs_ctx *ctx);


/* dof -> lattice location tables built by the library from the index pyramids:
 * 4 x int32 per DOF = (level | axis << 8, i, j, k).  kind selects velocity / edge / centre. */
avs_status avs_get_dof_table(avs_ctx *ctx, avs_index_kind kind, int32_t *table, avs_memspace where);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (the reference is single-process, so nothing here has a counterpart).
 * One process per GPU.  The octree is cut into spatial slabs along one axis (cuts on multiples of
 * 2^(levels-1) fine cells); every rank owns the rows of the faces inside its slab, renumbered
 * locally as [owned | halo grouped by owner]; per CG iteration the halo entries of p travel by
 * RCCL send/recv and the CG scalars by RCCL all-reduce, both enqueued on the solver's stream.
 *
 * Part 1 -- host-side planner (pure integer work on host arrays, usable without a GPU).
 * ---------------------------------------------------------------------------------------- */
typedef struct avs_plan avs_plan;
typedef struct {
    int64_t n_own, n_halo, nnz_local, n_send;
    int32_t n_peers;
} avs_plan_sizes;

/* owner rank of every velocity DOF: slabs along cut_axis balanced by row nnz */
avs_status avs_plan_owners(int64_t n, const int32_t *dof_table, const int32_t *row_ptr, int32_t levels,
                           int32_t cut_axis, int32_t extent_fine, int32_t world_size, int32_t *owner_out);
/* local structures of `rank`: owned rows, halo columns, local CSR pattern, send lists */
avs_status avs_plan_create(int64_t n, const int32_t *row_ptr, const int32_t *col, const int32_t *owner, int32_t rank,
                           int32_t world_size, avs_plan **out);
avs_status avs_plan_get_sizes(const avs_plan *plan, avs_plan_sizes *sizes);
/* own_global[n_own], halo_global[n_halo] (grouped by owner rank, ascending id), row_ptr_local[n_own+1],
 * col_local[nnz_local] (local ids: < n_own owned, else n_own + halo position), val_src[nnz_local]
 * (position of the entry in the global val array), peers[n_peers], send_counts / recv_counts[n_peers],
 * send_idx[n_send] (owned local ids, peer after peer).  Any pointer may be NULL. */
avs_status avs_plan_get_arrays(const avs_plan *plan, int32_t *own_global, int32_t *halo_global, int32_t *row_ptr_local,
                               int32_t *col_local, int32_t *val_src, int32_t *peers, int32_t *send_counts,
                               int32_t *recv_counts, int32_t *send_idx);
void avs_plan_destroy(avs_plan *plan);

/* ------------------------------------------------------------------------------------------
 * Part 2 -- device side.  Transport is RCCL (one process per GPU; the unique id is created on rank
 * 0 and broadcast by the host program, e.g. through torch.distributed) or, for single-GPU testing,
 * an in-process group of "virtual ranks" (one avs_ctx + one host thread each, same device).
 * ---------------------------------------------------------------------------------------- */
#define AVS_UNIQUE_ID_BYTES 128
avs_status avs_dist_get_unique_id(uint8_t id[AVS_UNIQUE_ID_BYTES]);
avs_status avs_dist_init(avs_ctx *ctx, const uint8_t id[AVS_UNIQUE_ID_BYTES], int32_t rank, int32_t world_size);

/* Hosted group: neither RCCL nor an in-process group -- the HOST PROGRAM carries the set-up data between the ranks (MPI, gloo,
 * files ...).  Only the direct transport (below) works in such a group.  Sequence on every rank: avs_dist_init_hosted,
 * avs_dist_assemble (or avs_assemble + avs_dist_partition), avs_dist_export_blob, exchange so that every rank holds all
 * blobs in rank order, avs_dist_import_blobs, avs_dist_solve.  avs_dist_get_solution then returns this rank's owned entries
 * (zeros elsewhere): the caller adds the per-rank vectors. */
#define AVS_DIST_BLOB_BYTES 512
avs_status avs_dist_init_hosted(avs_ctx *ctx, int32_t rank, int32_t world_size);
avs_status avs_dist_export_blob(avs_ctx *ctx, uint8_t blob[AVS_DIST_BLOB_BYTES]);
avs_status avs_dist_import_blobs(avs_ctx *ctx, const uint8_t *blobs /* world_size x AVS_DIST_BLOB_BYTES, rank order */);

typedef struct avs_local_group avs_local_group;
avs_status avs_local_group_create(int32_t world_size, avs_local_group **out);
void avs_local_group_destroy(avs_local_group *group);
avs_status avs_dist_init_local(avs_ctx *ctx, avs_local_group *group, int32_t rank);

/* Every rank calls it after avs_assemble on an identical (replicated) pyramid: keeps its slab of
 * the system (cut along `cut_axis`, -1 = longest axis) and builds halo / send lists.  The plan is built on the
 * device from the CSR in HBM; AVS_DIST_PLAN=host runs the host planner above on a downloaded copy instead
 * (identical arrays, kept as the reference for tests). */
avs_status avs_dist_partition(avs_ctx *ctx, int32_t cut_axis);
/* Distributed assembly ("each GPU assembles the rows it owns"): replaces avs_assemble + avs_dist_partition.
 * Every rank builds the cheap index-only pieces for the whole octree (dof tables, stress stencils, restriction, raw
 * triplet counts, brick-major permutation), picks the same slab cuts (balanced by raw triplet counts), then assembles,
 * sorts and compresses ONLY its own rows, and derives halo / send lists from them (the pattern is symmetric).  No
 * global matrix exists afterwards: avs_get_csr / avs_solve are unavailable, avs_dist_solve / avs_dist_get_solution work
 * as after avs_dist_partition.  info->nnz is the LOCAL non-zero count. */
avs_status avs_dist_assemble(avs_ctx *ctx, int32_t cut_axis, avs_assembly_info *info /* may be NULL */);
/* Slab-local path (round 6): the pre-pass of THIS rank's window + the assembly of its rows, nothing swept over the whole octree.
 *   avs_dist_bind_prepass(ctx, pp, cut_axis, cuts)   pp's next runs are slab-local (avs_prepass_set_slab with this rank, this group's
 *                                                     all-reduce -- RCCL or the in-process group; a hosted group passes its own callback
 *                                                     to avs_prepass_set_slab instead); cuts == NULL switches it off
 *   avs_prepass_run(pp, ...) ; avs_prepass_apply(pp, ctx) ; avs_dist_assemble(ctx, ...)      on every rank, collectively
 * The cuts must exist BEFORE anything is counted: take them from the previous frame -- avs_dist_get_cuts(ctx, 1, ...) returns the
 * cuts the last assembly's per-plane weights (summed over the ranks; a hosted group has no library-side exchange: it gets the cuts it
 * used) suggest for the next one, which = 0 the cuts it used -- or start from equal slabs.  avs_dist_assemble on such a context builds stencils for the stresses within 4 cells (of their level) of the
 * slab, the rank's rows (bit-identical to the reference's rows), halo and send lists; for the same cuts every array equals what the
 * replicated-index avs_dist_assemble produces.  Three lookup arrays indexed by DOF id (6 B per DOF, filled by memset) are the only
 * global-sized work.  avs_transfer_to_regular_grid(_in_place) on a slab-local context scatters and samples the DOFs of the rank's window
 * and writes the regular-grid faces whose position along the cut axis lies in the rank's slab (the others keep the input velocity);
 * it reads the WHOLE solution vector: avs_dist_get_solution first (it gathers it on every rank; hosted group: avs_set_solution).
 * Entries that need the whole pyramid (avs_assemble, avs_dist_partition) report AVS_ESTATE on a slab-local context. */
avs_status avs_dist_bind_prepass(avs_ctx *ctx, avs_prepass *pp, int32_t cut_axis, const int32_t *cuts /* world_size + 1, or NULL */);
avs_status avs_dist_get_cuts(avs_ctx *ctx, int32_t which, int32_t *cut_axis /* may be NULL */, int32_t *cuts /* world_size + 1 */);
avs_status avs_dist_get_plan_sizes(avs_ctx *ctx, avs_plan_sizes *sizes);
/* rows per SpMV tile (workgroup) of the solver's default kernel */
int32_t avs_spmv_tile_rows(void);
/* number of SpMV tiles that read no halo column (they run while the halo is in flight) / that do */
avs_status avs_dist_get_overlap_tiles(avs_ctx *ctx, int32_t *interior, int32_t *boundary);
/* the plan's arrays, copied to host memory (parity tests; sizes from avs_dist_get_plan_sizes / _overlap_tiles;
 * any pointer may be NULL): own_global[n_own], row_ptr_local[n_own+1], col_local[nnz_local], send_idx[n_send],
 * peers / send_counts / recv_counts[n_peers], tiles_interior[], tiles_boundary[] */
avs_status avs_dist_get_plan_arrays(avs_ctx *ctx, int32_t *own_global, int32_t *row_ptr_local, int32_t *col_local,
                                    int32_t *send_idx, int32_t *peers, int32_t *send_counts, int32_t *recv_counts,
                                    int32_t *tiles_interior, int32_t *tiles_boundary);
avs_status avs_dist_solve(avs_ctx *ctx, double tolerance, int32_t max_iterations, avs_solve_info *info);
/* how the partitioned solve of this context communicates (filled after avs_dist_partition / avs_dist_assemble) */
typedef enum {
    AVS_TRANSPORT_RCCL = 0,   /* k_pack + ncclSend/ncclRecv halo exchange, ncclAllReduce of the CG scalars */
    AVS_TRANSPORT_DIRECT = 1  /* peer-mapped comm blocks (IPC handles / peer access over xGMI): boundary entries are stored
                                 straight into the neighbour's halo area, CG scalars by a flag-based all-gather; no RCCL call
                                 inside the iteration */
} avs_dist_transport;
typedef struct {
    int32_t world_size;
    int32_t rccl_ranks;                /* ncclCommCount of the communicator; 0 = no RCCL communicator (in-process / hosted group) */
    int32_t transport;                 /* avs_dist_transport the next avs_dist_solve will use */
    int32_t graph_replay;              /* 1 = full chunks of iterations are replayed from a captured hipGraph */
    int32_t launches_per_iteration;    /* kernel launches per CG iteration of the loop in use */
    int32_t collectives_per_iteration; /* RCCL calls per CG iteration */
    int32_t selftest_rounds;           /* direct transport: pattern rounds run over the connected comm blocks before the first solve
                                          (AVS_DIST_SELFTEST_ROUNDS, default 64; 0 = not run) */
    int32_t paranoid;                  /* 1 = every round's halo segments are checked against the sender's checksum (AVS_DIST_PARANOID=1) */
    int64_t selftest_bad_entries;      /* all-gathered count of wrong halo entries / checksums in those rounds (0 = passed, -1 = not run,
                                          -2 = a wait timed out); a non-zero count retires the direct transport for the plan */
} avs_dist_info;
avs_status avs_dist_get_info(avs_ctx *ctx, avs_dist_info *info);
/* gathers the full solution (global DOF order) on every rank */
avs_status avs_dist_get_solution(avs_ctx *ctx, double *x, int64_t n, avs_memspace where);

#ifdef __cplusplus
}
#endif
#endif /* AVS_H */
