/* avs_probe.h -- measurement and test entries that are NOT part of the plugin seam (include/avs.h).  They are compiled (-DAVS_PROBES) into
 * libavs_probe.so only -- a superset build of libavs_hip.so from the same sources that also carries the SpMV kernel sweeps, the SELL and
 * stream probes and the fault-injection hooks (AVS_DIST_INJECT_STALE, AVS_CG_RESIDENT_FAKE_FAULT).  tools/ and the tests that need them
 * load that library; the product library exports none of this. */
#ifndef AVS_PROBE_H
#define AVS_PROBE_H
#include "avs.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One SpMV y = A x on device-resident CSR (measurement entry: the graded kernel).
 * `variant` selects the kernel (0 = library default).  Enqueues `repeats` launches. */
avs_status avs_spmv_csr(int64_t n, const int32_t *row_ptr, const int32_t *col, const double *val,
                        const double *x, double *y, int32_t variant, int32_t repeats, void *stream);
/* Measurement entry for the SELL-C-sigma experiment (C = 64: one wavefront per slice; BASELINE configs[4]): slice s holds 64
 * consecutive rows column-major, entry j of lane l at slice_ptr[s] + 64 j + l, padded with (col 0, val 0.0); device pointers.
 * y comes out in the slice (sigma-sorted) row order.  tools/sell_experiment.py builds the layout. */
avs_status avs_spmv_sell(int64_t nslices, const int64_t *slice_ptr, const int32_t *col, const double *val, const double *x,
                         double *y, int32_t repeats, void *stream, double *ms_per_launch);
/* SpMV on the system owned by ctx (after avs_assemble), same kernel the solver uses;
 * returns the mean HIP-event time per launch in *ms_per_launch. */
avs_status avs_bench_spmv(avs_ctx *ctx, int32_t variant, int32_t repeats, double *ms_per_launch);

/* y = A x with the storage form and kernel the solver's loop launches for the system owned by ctx (brick-structured form, word stream,
 * ...), for an ARBITRARY x: x and y are device vectors in the REFERENCE's DOF numbering (the entry permutes into the solver's brick-major
 * numbering and back).  fused_dot & 1 launches the fused-dot instantiation (what the PCG loop runs) and returns the folded x.y in
 * *dot_out.  The parity tests compare y with the CPU oracle's CSR product bit for bit.  A context assembled with
 * AVS_OPTION_MIXED_PRECISION = 1 multiplies with the mixed-precision loop's product (x narrowed to float, fp64 values and row sums, y
 * rounded to float); fused_dot & 2 asks such a context for the fp64 product of its reliable updates instead. */
avs_status avs_spmv_solver_form(avs_ctx *ctx, const double *x, double *y, int32_t fused_dot, double *dot_out);
/* the same for the LOCAL system of a partitioned solve (after avs_dist_assemble / avs_dist_partition): x_ext holds the rank's
 * [owned | halo] entries in local numbering (n_own + n_halo doubles, device), y its n_own rows.  A plan made with
 * AVS_OPTION_DIST_MIXED_PRECISION = 1 multiplies with the mixed-precision loops' product (all of x_ext narrowed to float, fp64 values and row
 * sums, y rounded to float); fused_dot & 2 asks such a plan for the fp64 product of its reliable updates instead. */
avs_status avs_dist_spmv_local_form(avs_ctx *ctx, const double *x_ext, double *y, int32_t fused_dot, double *dot_out);

/* y = A x on a caller's device CSR (reference numbering kept) with the lossless storage form avs_pcg_csr builds for it -- chosen under the
 * AVS_* environment of the call -- and the kernel the solve launches on that form.  *fmt (may be NULL; struct_size set by the caller) gets
 * value_table_size, column_bits, bytes_per_nonzero, tile_local_tables and column_windows of the form; the other fields are not written.
 * flags: AVS_SPMV_FORM_FUSED_DOT the fused-dot instantiation, the folded x.y in *dot_out; AVS_SPMV_FORM_F32 the float kernel of
 * AVS_PRECISION_F32 (x narrowed to float, y widened); AVS_SPMV_FORM_NO_CACHE_HINT the instantiation with non-temporal matrix loads, which
 * small matrices (those that fit the Infinity Cache) never reach otherwise. */
#define AVS_SPMV_FORM_FUSED_DOT 1
#define AVS_SPMV_FORM_F32 2
#define AVS_SPMV_FORM_NO_CACHE_HINT 4
avs_status avs_spmv_csr_form(int64_t n, const int32_t *row_ptr, const int32_t *col, const double *val, const double *x, double *y,
                             int32_t flags, double *dot_out, avs_matrix_format *fmt, void *stream);

/* avs_pcg_csr (same arguments, same solve, same AVS_* environment) + the CU-resident loop's plan for the caller's matrix: which of the
 * plan's edges the solve reached.  The caller sets struct_size; fields past it are not written.  `used`: the resident loop ran the solve
 * (= info->resident); otherwise `why` holds the reason (the plan's refusal, a refused cooperative launch, a timed-out wait) and the
 * counts hold what the plan had worked out before it stopped (0 where it had not got that far). */
typedef struct {
    int32_t struct_size;
    int32_t used;
    int32_t workgroups;             /* G: CUs the loop runs on (AVS_CG_RESIDENT_CUS) */
    int32_t max_lanes_per_workgroup;
    int64_t lanes;
    int32_t max_rows_per_workgroup;
    int32_t lc_bits;                /* workgroup-local column bits of the 25-bit word */
    int32_t ng;                     /* tier: row-local vectors kept in global memory (k_cg_resident<NG, ...>) */
    int32_t lds_bytes;
    int32_t max_quads;              /* register quads a lane uses (AVS_CG_RESIDENT_MAX_QUADS) */
    int32_t long_row_lanes;         /* lanes that hold one row longer than 5 max_quads words ... */
    int32_t longest_tail;           /* ... and the most words such a row leaves in memory */
    int32_t max_lane_streamed_rows; /* most streamed rows of one lane */
    int64_t streamed_rows;          /* > 0: the STREAM instantiation */
    int64_t streamed_words;
    int32_t max_remote;             /* most remote columns of a workgroup (its cache fill takes ceil(max_remote / 4096) trips) */
    int32_t remap_passes;           /* bitmap passes of the re-encoding kernel (AVS_CG_RESIDENT_REMAP_CHUNK) */
    int32_t local_tables;           /* the LT instantiation (AVS_RESIDENT_LOCAL_TABLES) */
    int32_t tables_per_workgroup;   /* 1, or 16: one per wave */
    int32_t largest_table;
    char why[128];
} avs_resident_plan_info;
avs_status avs_pcg_csr_plan(int64_t n, const int32_t *row_ptr, const int32_t *col, const double *val, const double *b, double *x,
                            double tol, int32_t max_iters, avs_memspace where, int32_t device, void *stream, avs_solve_info *info,
                            avs_resident_plan_info *plan);

/* The host half of that plan (csrc/avs_resident_plan.cpp) on HOST row pointers, without a device and without a HIP call: the lanes of the
 * n rows for `workgroups` workgroups with max_quads register quads per lane (1 .. 15), lane_fill and no_stream as AVS_CG_RESIDENT_LANE_FILL
 * (default 0.90) and AVS_CG_RESIDENT_NO_STREAM give them, then the plan's first split of the lanes into workgroups: by estimated time with
 * stream_cost (AVS_CG_RESIDENT_STREAM_COST, default 1.5) and no remote-column term, equal lanes where the clip at 1,024 lanes leaves some over.
 * lane_row0, lane_meta (register rows | streamed rows << 3 | a long row's words left in memory << 10) and lane_stream_quads have room for
 * n lanes, the first info->lanes are written; wg_lane0 and wg_row0 have workgroups + 1 entries.  A refusal of the planner is AVS_OK with
 * info->refused = 1 and its text in info->why; the arrays are not written then. */
typedef struct {
    int32_t struct_size;
    int32_t refused;
    int64_t lanes;
    int32_t long_row_lanes;
    int32_t longest_tail;
    int32_t max_lane_streamed_rows;
    int32_t max_rows_per_workgroup;
    int64_t streamed_rows;
    int64_t streamed_words;
    double stream_T;                /* streamed quads per lane the lanes were formed with (0: registers only) */
    char why[128];
} avs_resident_host_plan_info;
avs_status avs_resident_plan_host(int64_t n, const int32_t *row_ptr, int32_t workgroups, int32_t max_quads, double lane_fill, int32_t no_stream,
                                  double stream_cost, int32_t *lane_row0, uint32_t *lane_meta, int32_t *lane_stream_quads, int32_t *wg_lane0,
                                  int32_t *wg_row0, avs_resident_host_plan_info *info);

/* The integer geometry of a pre-pass run (csrc/avs_prepass_plan.cpp) without a device and without a HIP call, as avs_prepass_create and
 * avs_prepass_run plan it for an octree grid n[3] (powers of two) and desired_levels: the level cap of the extents, the ranges of every
 * level along the cut axis in level-l cells [lo, hi) -- win: the index window (avs_prepass_get_window), nl: the labels its classification
 * reads, v: the labels valid before the level serves as children, p1: the parents of octree pass 1 (levels >= 1) -- and the numbering's
 * tile layout: four batches (velocity faces, edges, centres over all levels, level-major then axis; the regular grid's three face
 * lattices) of 16^3-entry tiles behind each other, batch c at seg[c] with its tiles + 1 entries, then AVS_MAX_LEVELS level flags.
 * cuts (world + 1 entries from 0 to n[cut_axis], ascending) and world > 1 select the slab-local ranges of `rank`; cuts NULL or
 * world <= 1: every range is the whole level.  Entries of levels >= `levels` are 0. */
typedef struct {
    int32_t struct_size;
    int32_t levels;                                   /* min(desired_levels, what the extents carry) */
    int32_t win_lo[AVS_MAX_LEVELS], win_hi[AVS_MAX_LEVELS];
    int32_t nl_lo[AVS_MAX_LEVELS], nl_hi[AVS_MAX_LEVELS];
    int32_t v_lo[AVS_MAX_LEVELS], v_hi[AVS_MAX_LEVELS];
    int32_t p1_lo[AVS_MAX_LEVELS], p1_hi[AVS_MAX_LEVELS];
    int32_t level_tile0[4][AVS_MAX_LEVELS + 1];       /* first tile of every level inside batches 0 .. 2; [levels]: the batch's tiles */
    int32_t tile0_of[4][AVS_MAX_LEVELS][3];           /* first tile of lattice [level][axis] inside its batch (batch 3: level 0) */
    int64_t seg[5];                                   /* first entry of every batch in the count buffer */
    int64_t n_exchange;                               /* entries of the count buffer: what the ranks of a slab-local run sum */
} avs_prepass_plan_info;
avs_status avs_prepass_plan_host(const int32_t *n, int32_t desired_levels, int32_t cut_axis, const int32_t *cuts, int32_t world, int32_t rank,
                                 avs_prepass_plan_info *plan);

/* What the launch-per-phase loop (pcg_solve_phases, csrc/avs_pcg.hip) did in the LAST solve of the calling thread that ran it -- through
 * avs_pcg_csr, avs_pcg_csr_plan or avs_solve of this library --, so that a test which claims "graph replay" or "the alpha step as a
 * launch of its own" does not pass on a solve that took another way.  The caller sets struct_size; fields past it are not written.  Every
 * such solve starts a new record and adds 1 to `solves`; a solve the CU-resident loop took leaves the record of the solve before, so a
 * caller that must know compares `solves` before and after.  chunks_launched + chunks_replayed chunks were enqueued (a chunk: up to 32 iterations; what was enqueued past convergence
 * counts, the kernels of those iterations exit at once).  alpha_folded / alpha_launched count enqueued iterations by where their
 * alpha step ran: folded into the update_r launch, or as a reduction launch of its own; the iterations of a replayed chunk count as
 * the loop's launch-by-launch chunk before them did (every solve enqueues its first chunk launch by launch). */
typedef struct {
    int32_t struct_size;
    int32_t solves;            /* launch-per-phase solves of this thread so far */
    int32_t chunks_launched;   /* chunks enqueued launch by launch */
    int32_t chunks_replayed;   /* chunks replayed from a captured hipGraph */
    int32_t graphs_captured;   /* captures that were instantiated */
    int32_t graph_broken;      /* a capture failed on the solve's workspace: plain launches from then on */
    int32_t alpha_folded;
    int32_t alpha_launched;
    int32_t coded;             /* the vector kernels read 2-B diagonal codes and the table of inverted values */
    int32_t keep;              /* plain instead of non-temporal loads and stores in the vector kernels */
    int32_t fuse_beta;
    int32_t fuse_vectors;      /* the single fused vector launch was set up for this solve */
    int32_t g;                 /* workgroups of the vector kernels */
    int32_t nb;                /* partial sums the last enqueued SpMV leaves */
    int32_t float_vectors;     /* 0 fp64, 1 float vectors and scalars, 2 mixed precision */
    int32_t reserved;
} avs_phase_loop_report;
avs_status avs_phase_loop_info(avs_phase_loop_report *report);

/* Measurement: load balance of the brick kernel's row walk -- per G tile the quads of the slowest of the eight waves against the mean wave
 * (printed to stderr; out6 = {tiles, rows per tile, quads per row, slowest-wave quads, mean-wave quads, 0}) */
avs_status avs_brick_wave_stats(avs_ctx *ctx, double *out6);

/* Measured stream ceilings of the device for the access pattern of the SpMV's matrix stream
 * (mode 0: read-only 16 B/lane, 1: read-only non-temporal, 2: copy); GB/s of bytes moved. */
avs_status avs_bench_stream(int32_t mode, int64_t bytes, int32_t repeats, int32_t device, double *gbps);

/* The brick-structured SpMV form (csrc/avs_brick.hip) as plain device arrays, for a form built OUTSIDE the library
 * (tools/brick_build.py, the reference builder the device builder is tested against). */
typedef struct {
    int32_t ntiles;
    const uint32_t *tile_blk; /* 2 x uint32 per tile: first 16-B unit of its descriptor block, units */
    const uint32_t *blocks;   /* descriptor blocks (layout: csrc/avs_brick.hip) */
    const uint32_t *rdesc;    /* 2 x uint32 per pattern row (execution order): descriptor, position in the tile */
    const uint16_t *ownslot;  /* per row: own lattice slot in its tile, 0xffff none */
    const uint32_t *pwords;   /* global pattern words */
    const uint32_t *sdesc;    /* 2 x uint32 per streamed row: local row | len << 16, first word relative to the tile's */
    const uint32_t *swords;   /* streamed words (code << col_bits | column), CSR order */
    const double *table;      /* value dictionary */
    int32_t table_size, col_bits;
} avs_brick_arrays;
/* y = A x (+ per-wave partials of x.y when partial != NULL) with the brick kernel, `repeats` timed launches */
avs_status avs_brick_spmv_probe(const avs_brick_arrays *a, const double *x, double *y, double *partial, int32_t repeats, void *stream,
                                double *ms_per_launch);

/* The two vector kernels of one iteration of the launch-per-phase PCG loops -- update_r (r -= alpha A p, partial sums of r.r and r.z),
 * then update_xp (x += alpha p ; p = z + beta p) -- launched once each on the caller's device arrays with `g` workgroups (1 .. 2048).  The
 * product path reaches neither several trips per thread on a small grid nor the non-temporal instantiations below 200 MiB; this entry does.
 * flags: AVS_VECTOR_PROBE_F32 float vectors and float scalars (AVS_PRECISION_F32), AVS_VECTOR_PROBE_DS float vectors and double scalars (the
 * mixed-precision loop); neither: fp64.  AVS_VECTOR_PROBE_CODED: invd is the table of inverted values (as many entries as the codes reach)
 * and dcode holds a 2-B code per row, else invd has an entry per row and dcode may be NULL.  AVS_VECTOR_PROBE_KEEP: plain loads and stores
 * instead of non-temporal ones.  AVS_VECTOR_PROBE_FUSED: the kernels fold the partial sums and take the scalar steps themselves
 * (spmv_partial: nb partial sums of p.Ap); without it the scalars image holds what OP_ALPHA / OP_BETA leave (the float loops have a fused
 * update_xp only).  x, p, r, t and invd are arrays of the vector type (16-B aligned), vpart receives 2 g partial sums, `scalars` is a
 * device image of the library's PcgScalars (scalars_bytes must be its size: seven doubles rho, pAp, rr, alpha, beta, threshold, rhs_norm2,
 * four doubles of staging, the ints iter, done, fault, cancelled, the double rho_alt) and is updated in place.
 * AVS_VECTOR_PROBE_ONE_LAUNCH (with AVS_VECTOR_PROBE_FUSED, fp64 only): k_update_fused, the single launch with a grid barrier that
 * AVS_OPTION_FUSED_VECTOR_UPDATE puts in place of the pair, on the same arguments -- g must be 2048 and n at most 8,388,608 rows (else
 * AVS_EINVAL before anything is launched), nb 1 .. 4096, the device must have 256 CUs; the call returns when the launch has ended. */
#define AVS_VECTOR_PROBE_F32 1
#define AVS_VECTOR_PROBE_DS 2
#define AVS_VECTOR_PROBE_CODED 4
#define AVS_VECTOR_PROBE_KEEP 8
#define AVS_VECTOR_PROBE_FUSED 16
#define AVS_VECTOR_PROBE_ONE_LAUNCH 32
avs_status avs_vector_update_probe(int32_t flags, int32_t g, int64_t n, int32_t nb, int32_t parity, void *x, void *p, void *r, const void *t,
                                   const void *invd, const uint16_t *dcode, const double *spmv_partial, double *vpart, void *scalars,
                                   int32_t scalars_bytes, void *stream);

/* The scalar stages of the PCG loops (csrc/avs_pcg.hip, avs_halo.hpp, avs_pcg_mixed.inl) on the caller's device arrays: `launches` (1 .. 16)
 * back-to-back launches of the kernel `which` selects, on a device image of PcgScalars (layout and scalars_bytes as for
 * avs_vector_update_probe) that is updated in place.
 *   REDUCE_LAUNCH       reduce_launch's own choice between k_reduce and k_reduce_mb (the latter from 16,384 partial sums upward)
 *   REDUCE, REDUCE_MB   k_reduce at any nb >= 0, k_reduce_mb at any nb >= 1: `partial` holds nred arrays of nb sums, folded into
 *                       red[red_off .. red_off + nred); then the scalar op `op` (ScalarOp of avs_halo.hpp, 0: none) with `tol`
 *   REDUCE_PAIR         k_reduce_pair: red[0 .. nred) from `partial` (nb each), red[nred .. nred + nred_b) from partial_b (nb_b each)
 *   SCALAR              k_scalar: `op` alone
 *   MIXED_FINISH_INIT, MIXED_FINISH   k_mixed_finish<true> / <false> on 3 / 2 arrays of nb sums in `partial`
 *   SR_MIXED_BEGIN, SR_MIXED_STEP     k_sr_mixed_begin, k_sr_mixed_step
 * For REDUCE_LAUNCH and REDUCE_MB the entry owns the staging array and the ticket of k_reduce_mb, laid out as the solver's workspace lays
 * them out (64 x 4 doubles, one unsigned set to 0); slot i of the staging array starts as the NaN AVS_SCALAR_PROBE_STAGE_NAN | i.  After the
 * last launch the entry waits for the stream and returns the staging array in stage_out (HOST, 256 doubles, may be NULL) and the ticket in
 * *ticket_out (HOST, may be NULL; 0 for the other selectors). */
#define AVS_SCALAR_PROBE_REDUCE_LAUNCH 0
#define AVS_SCALAR_PROBE_REDUCE 1
#define AVS_SCALAR_PROBE_REDUCE_MB 2
#define AVS_SCALAR_PROBE_REDUCE_PAIR 3
#define AVS_SCALAR_PROBE_SCALAR 4
#define AVS_SCALAR_PROBE_MIXED_FINISH_INIT 5
#define AVS_SCALAR_PROBE_MIXED_FINISH 6
#define AVS_SCALAR_PROBE_SR_MIXED_BEGIN 7
#define AVS_SCALAR_PROBE_SR_MIXED_STEP 8
#define AVS_SCALAR_PROBE_STAGE_NAN 0x7ff8a5a500000000ull
avs_status avs_pcg_scalar_probe(int32_t which, const double *partial, int32_t nb, int32_t nred, const double *partial_b, int32_t nb_b,
                                int32_t nred_b, int32_t op, double tol, int32_t skip_if_done, int32_t red_off, int32_t launches,
                                void *scalars, int32_t scalars_bytes, double *stage_out, uint32_t *ticket_out, void *stream);

/* One launch of a vector kernel of the single-reduction loops on `g` workgroups (1 .. 2048) and the caller's device arrays:
 *   INIT                  k_sr_init: r = b - w, u = D^-1 r; partial: g sums each of b.b, r.u, r.r
 *   UPDATE                k_sr_update: p, s, x, r, u from w, alpha and beta; partial: g sums each of r.u, r.r.  step 1: the kernel first takes
 *                         the Chronopoulos-Gear step on scalars_in and workgroup 0 stores the new state in scalars_out (another image);
 *                         step 0: the scalars are used as they are (scalars_out may be scalars_in, and is not written)
 *   MIXED_RESIDUAL(_INIT) k_sr_mixed_residual<., false / true>: w holds the fp64 product t64 (doubles), r and u are float; partial: g sums
 *                         each of (INIT: b.b,) r.u, |b - t64|^2; scalars_in: the state whose `done` the plain form reads
 * flags (of avs_vector_update_probe): none fp64 vectors; F32 float vectors and scalars (INIT, UPDATE); DS float vectors, double scalars
 * (UPDATE); CODED with the float forms and the mixed residual: invd is the table of inverted values, dcode a 2-B code per row.  b is fp64
 * in every form; x, r, p, s, u, w (but for the mixed residual) and invd are arrays of the vector type; x, p, s are read by UPDATE only. */
#define AVS_SR_PROBE_INIT 0
#define AVS_SR_PROBE_UPDATE 1
#define AVS_SR_PROBE_MIXED_RESIDUAL 2
#define AVS_SR_PROBE_MIXED_RESIDUAL_INIT 3
avs_status avs_sr_vector_probe(int32_t kernel, int32_t flags, int32_t g, int64_t n, const double *b, void *x, void *r, void *p, void *s,
                               void *u, const void *w, const void *invd, const uint16_t *dcode, const void *scalars_in, void *scalars_out,
                               int32_t scalars_bytes, int32_t step, double *partial, void *stream);

/* The device setFromTriplets (csrc/avs_assembly.hip: k_wave_slots, k_unique_rows, k_unique_long, k_merge_rows, k_merge_long and the scans
 * between them) on the CALLER's triplets: n rows, raw_ptr[n + 1] plain row offsets (raw_ptr[0] == 0), raw_col / raw_val the triplets grouped
 * by row in emission order; all device pointers.  The entry lays them out the way the row sweep emits them -- a wave of 64 rows gets 64 x its
 * longest row, entry k of lane l at the wave's base + 64 k + l; the slots past a row's length are poisoned with a column of that row (0 for
 * an empty row) and a quiet NaN -- and then runs the functions avs_assemble runs on that layout: unique, scan, merge, merge-long.  f32 != 0:
 * duplicates are folded in float steps (AVS_PRECISION_F32; the values must be float values).  Columns are any int32 in [0, INT32_MAX - 1].
 * Results: row_ptr[n + 1], *nnz, and col / val when nnz <= capacity -- otherwise AVS_EINVAL, *nnz set, col / val untouched.
 * *info (struct_size set by the caller) gets the limits the kernels were compiled with and what the run reached.  With n == 0 and raw_ptr ==
 * row_ptr == NULL only the limits are filled in, and nothing touches the device (the CPU tests place their cases from them). */
typedef struct {
    int32_t struct_size;
    int32_t fast_limit;       /* kFast: rows up to here are merged in registers by their own thread */
    int32_t wave_limit;       /* rows up to here by their whole wave; longer ones go on the list of long rows */
    int32_t merge_lds;        /* kMergeLds: a wave's 64 merged rows are staged in LDS up to this many entries */
    int32_t scan_tile;        /* elements per workgroup of exclusive_scan_i32 (its top pass loops beyond 256 tiles) */
    int32_t long_grid_waves;  /* waves of the grids that walk the list of long rows */
    int32_t long_rows;        /* rows k_unique_rows listed */
    int32_t reserved;
    int64_t raw_slots;        /* slots of the wave-transposed raw arrays */
} avs_triplet_merge_info;
avs_status avs_merge_triplets_probe(int64_t n, const int32_t *raw_ptr, const int32_t *raw_col, const double *raw_val, int32_t f32,
                                    int32_t *row_ptr, int32_t *col, double *val, int64_t capacity, int64_t *nnz,
                                    avs_triplet_merge_info *info, void *stream);
/* exclusive_scan_i32 (the scan behind the assembly, the renumbering, the brick build, the pre-pass, the octree cells and the partition
 * plan) on device arrays: out[i] = in[0] + .. + in[i - 1] for i <= n.  A total above INT32_MAX comes back as out[n] == -1, and then only
 * out[n] is defined. */
avs_status avs_exclusive_scan_probe(const int32_t *in, int32_t *out /* n + 1 */, int64_t n, void *stream);
/* The context's AVS_FIELD_VISCOSITY as the assembly reads it: *is_const = 1 and *constant, or *is_const = 0 and, if lattice is not NULL,
 * the padded centre lattice (nx*ny*nz floats, x fastest) -- what avs_set_scalar_field or avs_apply_viscosity_model(install) left there. */
avs_status avs_viscosity_lattice_probe(avs_ctx *ctx, float *lattice /* may be NULL */, float *constant, int32_t *is_const, avs_memspace where);

/* The brick-structured SpMV form (csrc/avs_brick_build.hip: build_brick_form(BrickForm &, const BrickSource &, ...), the function the solver
 * and the partitioned plan call) and its kernel (csrc/avs_brick.hip: k_spmv_brick) on the CALLER's system: a device CSR of n_rows rows and
 * n_cols >= n_rows columns (columns >= n_rows are halo columns, as in a partitioned rank's local system), one dof record per COLUMN in the
 * int4 layout k_bk_geo reads (level | axis << 8, i, j, k; device, 4 n_cols int32), the grid nx, ny, nz (<= 1024 each) and its levels.  The
 * rows must already be brick-major (brick ids non-decreasing): the entry uses an identity ref_id and reorders nothing.  It builds the value
 * index as avs_spmv_csr_form does (build_matrix_index under the AVS_* environment of the call), the form under the Options of that
 * environment (AVS_BRICK, AVS_BRICK_MIN_REGULAR, ...), and launches the kernel the loops launch: y = A x for device vectors x (n_cols
 * doubles) and y (n_rows doubles).
 * flags: FUSED_DOT the fused-dot instantiation (x.y folded in partial order in *dot_out; the per-workgroup partials in `partials`, a HOST
 * array of partial_capacity doubles, may be NULL: the device array is initialised from it and copied back, so slots the launch does not
 * write keep the caller's values); F32 the float kernel (x narrowed to float, y widened; the matrix values must be float values); MIXED
 * k_spmv_brick<.., float, double> (x narrowed, y widened); VALUE_CODES forces the value-code variant (the form is built without a value
 * dictionary); DONE (with FUSED_DOT only: the plain instantiation has no flag) hands the launch a device flag set to 1 -- it must leave y
 * and the partials untouched.
 * grid: 0 the library's default, otherwise the persistent grid (the library clamps either to the number of tiles).  walk: 0 contiguous
 * eighths, 1 dealt chunks, 2 the planned walk (BrickForm::plan_walk for that grid over dealt chunks; it plans nothing unless the grid is a
 * multiple of 8, at most the tiles, and every workgroup gets a tile -- info->planned says whether it did).
 * *info (struct_size set by the caller) gets the limits the code was compiled with and what the build made; `headers` (HOST, may be NULL)
 * the first 16 header words of every tile's descriptor block in tile-list order when tiles <= header_capacity.  With n_rows == 0 and
 * row_ptr == NULL only the limits are filled in and nothing touches the device (the CPU tests place their cases from them).
 * Refused with AVS_EINVAL on the host, before any launch: an empty row (the assembled systems always hold a diagonal, and the kernel does
 * not write y for a streamed row of length 0), rows not in brick order, a column outside [0, n_cols), a dof record the geometry key cannot
 * hold.  A form that is not ready is AVS_OK with info->ready == 0, no product, and the counts that were worked out. */
#define AVS_BRICK_PROBE_FUSED_DOT 1
#define AVS_BRICK_PROBE_F32 2
#define AVS_BRICK_PROBE_MIXED 4
#define AVS_BRICK_PROBE_VALUE_CODES 8
#define AVS_BRICK_PROBE_DONE 16
typedef struct {
    int32_t struct_size;
    /* limits */
    int32_t run_len;          /* kBrickRunLen */
    int32_t max_runs;         /* kBrickMaxRuns */
    int32_t fast_runs;        /* kRuFast * QW: fill runs held in registers */
    int32_t pat_max;          /* kBrickPatMax */
    int32_t pat_words;        /* kBrickPatWords */
    int32_t pat_words_vc;     /* kBrickPatWordsVc */
    int32_t pat_len;          /* kBrickPatLen */
    int32_t x_slots;          /* kBrickXSlots */
    int32_t park_words;       /* kBrickPark - kBrickXSlots: streamed products per pass of a G tile */
    int32_t emode_words;      /* ... of a tile without patterns (fp64 and float kernels) */
    int32_t emode_words_mixed;/* ... in the mixed kernel */
    int32_t min_rows;         /* kBrickMinRows */
    int32_t max_rows;         /* kBrickMaxRows */
    int32_t etile_rows;       /* kBrickETileRows */
    int32_t tile_vals;        /* kBrickTileVals */
    int32_t table_max;        /* kBrickTableMax */
    int32_t block_words;      /* words reserved per descriptor block */
    int32_t header_words;     /* kBlkHdrWords */
    /* the build */
    int32_t ready, vc, wide, col_bits;
    int32_t tiles, patterns, halo_tiles;
    int32_t grid;             /* workgroups launched */
    int32_t max_walk;         /* most tiles any workgroup walks */
    int32_t planned;          /* walk 2: plan_walk laid the walk out */
    int32_t table_size;       /* of the value dictionary (0: value-code variant) */
    int32_t reserved;
    int64_t pattern_rows, streamed_rows, streamed_words;
} avs_brick_form_info;
avs_status avs_brick_form_probe(int64_t n_rows, int64_t n_cols, const int32_t *row_ptr, const int32_t *col, const double *val,
                                const int32_t *dof, int32_t nx, int32_t ny, int32_t nz, int32_t levels, const double *x, double *y,
                                int32_t flags, int32_t grid, int32_t walk, double *dot_out, double *partials, int32_t partial_capacity,
                                avs_brick_form_info *info, int32_t *headers, int32_t header_capacity, void *stream);

/* The device partition planners (csrc/avs_dist_plan.hip) on the CALLER's arrays: the functions avs_dist_partition and avs_dist_assemble call,
 * without a context.  All inputs are device arrays, every result is copied to a HOST array of a stated capacity (any may be NULL).
 *   PLAN  plan_from_source, the core of avs_dist_partition's device planner: a CSR of n rows (any columns in [0, n), any row lengths
 *         including 0, duplicates allowed, the pattern need not be symmetric), its values, one int4 dof record per DOF (level | axis << 8,
 *         i, j, k), perm (row i stands for the DOF perm[i]; NULL: identity), levels (1 .. 8), cut_axis, extent (>= 1, any value that gives
 *         at most 65,535 planes of 2^(levels-1) cells -- not tied to the 1,024 limit of a grid), rank and world.
 *   TAIL  dist_tail_from_rows, everything avs_dist_assemble does behind assemble_rows: a CSR over n ids whose PATTERN IS SYMMETRIC, `owner`
 *         (one byte per id: its rank, 0xFF: outside the rank's window), rank, world, split (!= 0: [interior | halo-reading] local row order)
 *         and dom (NULL: every id; else n_dom <= n distinct ids, the only ones a halo column may have, in the order halo ids are numbered
 *         in).  The entry gathers the rows whose owner is `rank` in ascending id order -- the state after assemble_rows, the right-hand
 *         side of row i being (double)i -- and calls the core with identity inv / perm.  A column whose owner is 0xFF comes back as the
 *         core's AVS_EINTERNAL.
 * Results (out): weights and plane_owner per plane and owner per row (PLAN only); own_global (TAIL: in the possibly reordered local order),
 * halo_global, row_ptr_local (n_own + 1), col_local, val_local, send_idx (grouped by peer), peers / send_counts / recv_counts (room for 32
 * each), tiles_int, tiles_bnd, and for TAIL local_ref (n_own + n_halo) and rhs_local.  row_capacity bounds n_own, n_halo, n_own + n_halo
 * (local_ref) and the tile lists; nnz_capacity, send_capacity and plane_capacity the others: a result beyond its capacity is AVS_EINVAL with
 * the sizes in *info.
 * In the probe every array the planner fills is allocated with 64 guard bytes of a known pattern behind its last entry (the product's
 * allocations are not changed: the cores allocate through one helper that is DevBuf::alloc / reserve without guards);
 * info->guard_bytes_hit counts the guard bytes that were altered.
 * *info (struct_size set by the caller) gets the limits the code was compiled with and the sizes of the plan.  With in == NULL, or in->n == 0
 * and in->row_ptr == NULL, only the limits are filled in and nothing touches the device (the CPU tests place their cases from them).
 * Refused with AVS_EINVAL on the host, before any launch: rank >= world, world > 32, levels / cut_axis / extent out of range, row pointers
 * that do not start at 0 or decrease, a column outside [0, n), a dof record whose level exceeds 30 or whose coordinate is negative, a perm
 * or dom entry outside [0, n), an owner byte that is neither < world nor 0xFF, and in TAIL mode an asymmetric pattern. */
#define AVS_DIST_PLAN_PROBE_PLAN 0
#define AVS_DIST_PLAN_PROBE_TAIL 1
typedef struct {
    int64_t n;
    const int32_t *row_ptr, *col;
    const double *val;
    const int32_t *dof, *perm;      /* PLAN */
    const uint8_t *owner;           /* TAIL */
    const int32_t *dom;             /* TAIL */
    int64_t n_dom;
    int32_t levels, cut_axis, extent; /* PLAN */
    int32_t split;                  /* TAIL */
    int32_t rank, world;
} avs_dist_plan_input;
typedef struct {
    int64_t row_capacity, nnz_capacity, send_capacity, plane_capacity;
    int64_t *weights;
    int32_t *plane_owner;
    uint8_t *owner;                 /* n entries */
    int32_t *own_global, *halo_global, *row_ptr_local, *col_local;
    double *val_local;
    int32_t *send_idx, *peers, *send_counts, *recv_counts, *tiles_int, *tiles_bnd, *local_ref;
    double *rhs_local;
} avs_dist_plan_output;
typedef struct {
    int32_t struct_size;
    /* limits */
    int32_t lds_planes;             /* kPlanLdsPlanes: more planes than this are weighed with global atomics */
    int32_t scan_tile;              /* elements per workgroup of exclusive_scan_i32 */
    int32_t spmv_tile_rows;         /* avs_spmv_tile_rows(): rows per entry of the tile lists */
    int32_t row_group;              /* lanes that share a row in the mark / localize / move kernels */
    int32_t max_world;
    /* the plan */
    int32_t nplanes, n_peers, n_tiles_int, n_tiles_bnd;
    int64_t n_own, n_halo, n_send, nnz_local;
    int64_t n_interior;             /* TAIL with a split: rows that read no other rank; else -1 */
    int64_t guard_bytes_hit;
} avs_dist_plan_info;
avs_status avs_dist_plan_probe(int32_t mode, const avs_dist_plan_input *in, const avs_dist_plan_output *out, avs_dist_plan_info *info,
                               void *stream);


#ifdef __cplusplus
}
#endif
#endif
