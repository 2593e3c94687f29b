// avs_host.hpp -- C++ host side above the C ABI (include/avs.h).
//
// Mirrors the hot-path slice of HDK_AdaptiveViscosity::solveGasSubclass (HDK_AdaptiveViscosity.cpp,
// "cpp:") with the reference's own phase names, on plain dense arrays instead of SIM_Raw*Field:
//
//   reference (cpp)                                   here
//   ------------------------------------------------  ------------------------------------------
//   octreeLabels.getGridLabels(level)       oct.h:144  setOctreeLabels(level, ...)
//   octreeVelocityIndices / edgeStressIndices /       setOctreeVelocityIndices / setEdgeStressIndices /
//   centerStressIndices                  cpp:337-393  setCenterStressIndices + setDOFCounts
//   buildEdgeStressStencils, buildCenterStress*       buildStressStencils()            cpp:443-498
//   buildVelocityMapping                 cpp:518-528  buildVelocityMapping()
//   buildOctreeSystemFromStencils + setFromTriplets   buildOctreeSystemFromStencils()  cpp:577-593, 613-614
//   ConjugateGradient::solveWithGuess    cpp:618-630  solveConjugateGradient(tol, maxIterations)
//   regularVelocityIndices               cpp:303-329  setRegularVelocityIndices(axis, ...)
//   setOctreeVelocity + interpolator +
//   applyVelocitiesToRegularGrid         cpp:661-707  applyVelocitiesToRegularGrid(u, v, w)
//
// Header-only; needs only include/avs.h and -lavs_hip.  Errors of the C ABI become std::runtime_error
// (the reference returns false after addError; Houdini-side glue is in INTEGRATION.md).
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "avs.h"

namespace avs_host {

struct SolveResult {
    int iterations = 0;
    bool converged = false;
    double error = 0.;
    double solveMs = 0., spmvMs = 0.;
};

class AdaptiveViscosity {
public:
    // nx, ny, nz: padded octree resolution; fieldRes: the simulation grid the scalar fields live on (oct.cpp:13-24),
    // nullptr = the same
    AdaptiveViscosity(int nx, int ny, int nz, double dx, double dt, int octreeLevels, bool useEnhancedGradients = true,
                      int device = 0, const int *fieldRes = nullptr, int solveType = AVS_PRECISION_F64)
    {
        avs_desc d{};
        d.nx = nx; d.ny = ny; d.nz = nz;
        if (fieldRes) { d.field_nx = fieldRes[0]; d.field_ny = fieldRes[1]; d.field_nz = fieldRes[2]; }
        d.dx = dx; d.dt = dt;
        d.levels = octreeLevels;
        d.use_enhanced_gradients = useEnhancedGradients ? 1 : 0;
        d.device = device;
        d.stream = nullptr;
        d.precision = solveType; // SolveType of the reference build (util.h:25-37): fpreal64, or fpreal32 under USESINGLEPRECISION
        check(avs_create(&d, &myCtx), "avs_create");
        myLevels = octreeLevels;
    }
    ~AdaptiveViscosity() { avs_destroy(myCtx); }
    AdaptiveViscosity(const AdaptiveViscosity &) = delete;
    AdaptiveViscosity &operator=(const AdaptiveViscosity &) = delete;

    // ---- inputs produced by cpp:233-416 -----------------------------------------------------------
    void setOctreeLabels(int level, const int8_t *labels) { check(avs_set_labels(myCtx, level, labels, AVS_MEM_HOST), "labels"); }
    void setOctreeVelocityIndices(int level, int axis, const int32_t *idx) { setIndex(AVS_INDEX_VELOCITY, level, axis, idx); }
    void setEdgeStressIndices(int level, int axis, const int32_t *idx) { setIndex(AVS_INDEX_EDGE, level, axis, idx); }
    void setCenterStressIndices(int level, const int32_t *idx) { setIndex(AVS_INDEX_CENTER, level, 0, idx); }
    void setDOFCounts(int64_t octreeVelocityDOFCount, int64_t edgeStressDOFCount, int64_t centerStressDOFCount)
    {
        check(avs_set_dof_counts(myCtx, octreeVelocityDOFCount, edgeStressDOFCount, centerStressDOFCount), "dof counts");
    }
    // data == nullptr: constant field (HDK field()->isConstant fast path)
    void setField(avs_field_kind kind, int axis, const float *data, float constant = 0.f)
    {
        check(avs_set_scalar_field(myCtx, kind, axis, data, constant, AVS_MEM_HOST), "field");
    }

    // solver switches (avs_set_solver_option): e.g. (AVS_OPTION_PRECONDITIONER, AVS_PRECONDITIONER_NONE) = the build without USEEIGEN
    // (cpp:633-642); (AVS_OPTION_RESIDENT_LOOP, 0) on a GPU shared with a viewport; (AVS_OPTION_BRICK_FORM, AVS_BRICK_NEVER)
    void setSolverOption(avs_solver_option option, int value) { check(avs_set_solver_option(myCtx, option, value), "avs_set_solver_option"); }

    // ---- hot path ---------------------------------------------------------------------------------
    void buildStressStencils() { check(avs_build_stencils(myCtx), "buildStressStencils"); }
    void buildVelocityMapping() { check(avs_build_initial_guess(myCtx), "buildVelocityMapping"); }
    void buildOctreeSystemFromStencils() { check(avs_build_system(myCtx), "buildOctreeSystemFromStencils"); }
    avs_assembly_info buildLinearSystem()
    {
        avs_assembly_info info{};
        check(avs_assemble(myCtx, &info), "avs_assemble");
        return info;
    }
    // is the assembled system one the solve is defined for? (avs_check_system: pointers, columns, finite values, ascending rows, a
    // positive diagonal, symmetry within an absolute tolerance; report.passed, and the measured asymmetry of A)
    avs_csr_check checkLinearSystem(uint32_t what = AVS_CSR_CHECK_ALL, double symmetryTolerance = 0.)
    {
        avs_csr_check report{};
        report.struct_size = (int32_t)sizeof(report);
        check(avs_check_system(myCtx, what, symmetryTolerance, &report), "avs_check_system");
        return report;
    }
    // are the edge and centre stress index pyramids ones the hot path is defined for? (avs_check_stress_indices: where the reference
    // asserts edgeStressUnitTest and centerStresUnitTest, cpp:412-413; report.passed, a count per rule and the first violating entry)
    avs_stress_check checkStressIndices(uint32_t what = AVS_CHECK_EDGE_INDICES | AVS_CHECK_CENTER_INDICES)
    {
        avs_stress_check report{};
        report.struct_size = (int32_t)sizeof(report);
        check(avs_check_stress_indices(myCtx, what, &report), "avs_check_stress_indices");
        return report;
    }
    // the deformation of the solution (AVS_RATES_OF_SOLUTION) or of the restricted input velocity (AVS_RATES_OF_INITIAL_GUESS: after
    // buildStressStencils + buildVelocityMapping, before any system exists): the rate of every edge stencil and centre list, the shear
    // rate sqrt(2 eps:eps) of every ACTIVE cell by centre id, and the summary (avs_get_strain_rates; counters, dissipations, maxima)
    struct StrainRates {
        std::vector<double> edge, center, cell;
        avs_strain_summary summary{};
    };
    StrainRates strainRates(int32_t which = AVS_RATES_OF_SOLUTION)
    {
        StrainRates r;
        r.summary.struct_size = (int32_t)sizeof(r.summary);
        check(avs_get_strain_rates(myCtx, which, nullptr, nullptr, nullptr, &r.summary, AVS_MEM_HOST), "avs_get_strain_rates");
        r.edge.resize((size_t)r.summary.n_edge);
        r.center.resize(3 * (size_t)r.summary.n_center);
        r.cell.resize((size_t)r.summary.n_center);
        check(avs_get_strain_rates(myCtx, which, r.edge.data(), r.center.data(), r.cell.data(), nullptr, AVS_MEM_HOST), "avs_get_strain_rates");
        return r;
    }
    // the shear rate on the simulation grid (field_nx * field_ny * field_nz floats, x fastest: the lattice of AVS_FIELD_VISCOSITY), 0 where
    // no ACTIVE cell covers a cell -- what a shear-dependent viscosity mu(gamma) is evaluated from
    void shearRateField(float *field, int32_t which = AVS_RATES_OF_SOLUTION)
    {
        check(avs_get_shear_rate_field(myCtx, which, field, AVS_MEM_HOST), "avs_get_shear_rate_field");
    }
    // a shear-dependent viscosity evaluated on the device (avs_apply_viscosity_model: Carreau-Yasuda or Herschel-Bulkley of the cells'
    // shear rates, the liquid's values continued one cell into the air, relaxation against the current viscosity).  field: field_nx *
    // field_ny * field_nz floats on the host, or null.  install: the result becomes AVS_FIELD_VISCOSITY on the device, as setField with
    // it would -- stencils, system and solution are gone afterwards.  summary.max_relative_change is the stopping measure of a
    // fixed-point loop.
    avs_viscosity_summary applyViscosityModel(avs_viscosity_model model, int32_t which = AVS_RATES_OF_SOLUTION, bool install = false,
                                              float *field = nullptr)
    {
        model.struct_size = (int32_t)sizeof(model);
        avs_viscosity_summary summary{};
        summary.struct_size = (int32_t)sizeof(summary);
        check(avs_apply_viscosity_model(myCtx, which, &model, field, install ? 1 : 0, &summary, AVS_MEM_HOST), "avs_apply_viscosity_model");
        return summary;
    }
    // the fixed-point (Picard) loop over it; declared behind solveConjugateGradient
    struct ShearDependentSolve {
        bool converged = false;
        avs_viscosity_summary initial{};              // the evaluation on the restricted input velocity
        std::vector<SolveResult> solves;              // one per solve
        std::vector<avs_viscosity_summary> summaries; // the evaluation on each solve's solution
    };
    // did x solve the assembled system? (avs_check_solution: the true b - A x in fp64 from the plain CSR, whatever loop and storage form
    // produced x; report.relative_residual next to report.claimed_error, the solve's own figure.)  residual: n doubles on the host, or
    // null.  which = AVS_CHECK_OF_INITIAL_GUESS: the residual the solve starts from.
    avs_solution_check checkSolution(int32_t which = AVS_CHECK_OF_SOLUTION, double *residual = nullptr)
    {
        avs_solution_check report{};
        report.struct_size = (int32_t)sizeof(report);
        check(avs_check_solution(myCtx, which, residual, &report, AVS_MEM_HOST), "avs_check_solution");
        return report;
    }
    // why does the solve take the iterations it takes? (avs_estimate_spectrum: `steps` Lanczos steps in fp64 on the Jacobi-scaled matrix
    // -- op = AVS_SPECTRUM_OF_MATRIX: on A -- started from the scaled initial residual.  report.lambda_min / lambda_max with their
    // bounds, report.condition_estimate (a lower bound), report.iteration_bound for `tolerance`, report.indefinite.)  ritz: `steps`
    // doubles on the host, or null.  Needs avs_assemble; changes nothing a later solve reads.
    avs_spectrum estimateSpectrum(int32_t steps = 32, double tolerance = 1e-3, int32_t op = AVS_SPECTRUM_OF_JACOBI, double *ritz = nullptr)
    {
        avs_spectrum report{};
        report.struct_size = (int32_t)sizeof(report);
        check(avs_estimate_spectrum(myCtx, op, AVS_SPECTRUM_START_RESIDUAL, steps, tolerance, nullptr, nullptr, ritz, nullptr, nullptr, AVS_MEM_HOST, &report),
              "avs_estimate_spectrum");
        return report;
    }
    SolveResult solveConjugateGradient(double solverTolerance = 1e-3, int maxSolverIterations = 2500)
    {
        avs_solve_info s{};
        check(avs_solve(myCtx, solverTolerance, maxSolverIterations, &s), "avs_solve");
        SolveResult r;
        r.iterations = s.iterations;
        r.converged = s.converged != 0;
        r.error = s.error;
        r.solveMs = s.solve_ms;
        r.spmvMs = s.spmv_ms;
        myDofs = s.n;
        return r;
    }
    // Provisional fields set: the model is evaluated on the restricted input velocity and installed; then assemble, solve, evaluate on
    // the solution WITHOUT installing; max_relative_change <= picardTolerance ends the loop, else the same evaluation is installed and
    // the loop goes again (at most maxPicard solves).  No field crosses the bus.  On return the context is solved by the system that
    // produced its solution: the transfer and checkSolution work.
    ShearDependentSolve solveShearDependent(const avs_viscosity_model &model, double solverTolerance = 1e-3, int maxSolverIterations = 2500,
                                            double picardTolerance = 1e-3, int maxPicard = 20)
    {
        ShearDependentSolve r;
        buildStressStencils();
        buildVelocityMapping();
        r.initial = applyViscosityModel(model, AVS_RATES_OF_INITIAL_GUESS, true);
        for (int k = 0; k < (maxPicard > 1 ? maxPicard : 1); ++k) {
            buildLinearSystem();
            r.solves.push_back(solveConjugateGradient(solverTolerance, maxSolverIterations));
            r.summaries.push_back(applyViscosityModel(model, AVS_RATES_OF_SOLUTION, false));
            if (r.summaries.back().max_relative_change <= picardTolerance) {
                r.converged = true;
                break;
            }
            if (k + 1 < maxPicard) applyViscosityModel(model, AVS_RATES_OF_SOLUTION, true); // the same values, now the context's field
        }
        return r;
    }
    std::vector<double> viscositySolution() const
    {
        std::vector<double> x((size_t)myDofs);
        check(avs_get_solution(myCtx, x.data(), myDofs, AVS_MEM_HOST), "avs_get_solution");
        return x;
    }
    // ---- post-solve transfer, cpp:655-707 ----------------------------------------------------------
    void setRegularVelocityIndices(int axis, const int32_t *idx)
    {
        check(avs_set_regular_index_field(myCtx, axis, idx, AVS_MEM_HOST), "regular index field");
    }
    // u: (nx+1)*ny*nz, v: nx*(ny+1)*nz, w: nx*ny*(nz+1) floats, x fastest
    void applyVelocitiesToRegularGrid(float *u, float *v, float *w)
    {
        check(avs_transfer_to_regular_grid(myCtx, u, v, w, AVS_MEM_HOST), "applyVelocitiesToRegularGrid");
    }
    // the same as an in-place update of a DEVICE-resident velocity field (what the reference does to `vel`, cpp:655-707): the arrays already
    // hold what was given as AVS_FIELD_VELOCITY; only the faces the transfer changes are written
    void applyVelocitiesToRegularGridInPlace(float *d_u, float *d_v, float *d_w)
    {
        check(avs_transfer_to_regular_grid_in_place(myCtx, d_u, d_v, d_w), "applyVelocitiesToRegularGridInPlace");
    }
    int octreeLevels() const { return myLevels; }
    avs_ctx *handle() const { return myCtx; }

private:
    void setIndex(avs_index_kind kind, int level, int axis, const int32_t *idx)
    {
        check(avs_set_index_field(myCtx, kind, level, axis, idx, AVS_MEM_HOST), "index field");
    }
    static void check(avs_status s, const char *what)
    {
        if (s != AVS_OK) throw std::runtime_error(std::string(what) + ": " + avs_last_error());
    }
    avs_ctx *myCtx = nullptr;
    int myLevels = 0;
    int64_t myDofs = 0;
};

} // namespace avs_host
