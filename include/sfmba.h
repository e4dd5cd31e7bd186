/*
 * sfmba.h -- C ABI of the MI355X-native bundle-adjustment back end that drops in
 * behind sfmtoylib::SfMBundleAdjustmentUtils::adjustBundle().
 *
 * Reference interface replaced (all paths relative to the reference checkout):
 *   SfMToyLib/SfMBundleAdjustmentUtils.h:44-49    adjustBundle() declaration
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:58-97  SimpleReprojectionError (2 residuals; 6/3/1 params)
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:171-179 ceres::Solver::Options + ceres::Solve
 *   SfMToyLib/SfMBundleAdjustmentUtils.cpp:182-185 termination gate (only CONVERGENCE is written back)
 *
 * The reference has no FFI: its "operator API" for this path is the single static C++
 * function above, whose body hands flat double arrays (camera 6-vectors, 3D points, one
 * shared focal) to ceres::Problem / ceres::Solve.  This header is the boundary a
 * maintainer binds instead of Ceres: plain pointers and sizes, no C++/torch types.
 * The C++ shim that keeps the reference signature lives in
 * sfm-toy-library_amd/host/SfMBundleAdjustmentUtils.cpp.
 *
 * Conventions
 *   camera j : cam6[6*j+0..2] = angle-axis (Rodrigues) rotation, cam6[6*j+3..5] = translation,
 *              world->camera: p = Rot(w) * X + t                      (BA.cpp:67-74)
 *   point i  : pt3[3*i+0..2]
 *   focal    : one scalar shared by every camera                      (BA.cpp:92,138,164)
 *   obs k    : (obs_cam[k], obs_pt[k], obs_xy[2k], obs_xy[2k+1]) with the principal point
 *              already subtracted                                     (BA.cpp:149-153)
 *   residual : r = focal * (p.x/p.z, p.y/p.z) - obs                   (BA.cpp:76-86)
 *   cost     : 1/2 * sum ||r||^2  (Ceres convention)
 * Cameras/points that no observation references are not part of the problem and are
 * left untouched (Ceres only sees parameter blocks passed to AddResidualBlock, BA.cpp:160).
 */
#ifndef SFMBA_H_
#define SFMBA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFMBA_ABI_VERSION 6

#if defined(__GNUC__)
#define SFMBA_API __attribute__((visibility("default")))
#else
#define SFMBA_API
#endif

/* ceres::TerminationType values the reference tests against (BA.cpp:182). */
enum {
    SFMBA_CONVERGENCE    = 0,
    SFMBA_NO_CONVERGENCE = 1,
    SFMBA_FAILURE        = 2
};

enum { SFMBA_LINEAR_CHOLESKY = 0,   /* exact Schur + dense LLT == DENSE_SCHUR (BA.cpp:172), always factorised */
       SFMBA_LINEAR_PCG      = 1,   /* exact Schur + two-level block-Jacobi PCG on the dense reduced system, stopped at pcg_tolerance
                                       (inexact Newton: parameters agree with the exact solve to ~1e-8, cost to 1e-12) */
       SFMBA_LINEAR_AUTO     = 2 }; /* THE DEFAULT (library and drop-in shim): the reference's DENSE_SCHUR result at the cost of the
                                       cheapest solver that delivers it.  Up to 256 reduced unknowns (the reference's own data sets):
                                       CHOLESKY.  Above: the same PCG run to a plain relative residual of min(pcg_tolerance, 1e-12)
                                       -- the step then agrees with the factorised solve to ~1e-10 relative, below what the float
                                       containers of adjustBundle() resolve -- and, if the CG has not converged after
                                       pcg_max_iters (0 = min(4 dim, 200)) iterations, the SAME linearisation is solved by CHOLESKY
                                       instead (the matrix is re-formed unpreconditioned; nothing is skipped).  A CG that BREAKS DOWN
                                       (non-positive curvature, NaN) is not retried: the step is invalid, exactly as after a failed
                                       factorisation (radius halved, FAILURE after five in a row).  A linearisation that needed more
                                       CG iterations than a factorisation costs (~3.3 per block column of 64) makes the following
                                       ones OF THE SAME SOLVE go straight to CHOLESKY (the preference is not remembered across
                                       solves: a resident problem solved twice from the same point takes the same path twice).
                                       Sharded solves (sfmba_problem_solve_sharded, sfmba_shard_*) have no fallback: AUTO there is the
                                       CG at 1e-12 with the step forced at pcg_max_iters.  Above 1280 reduced unknowns in
                                       SFMBA_PRECISION_F32J the CG iterates on an fp32-rounded copy of the preconditioned matrix
                                       (pcg_f32_matrix = -1 keeps fp64): the converged step is that of the rounded matrix, ~1e-7
                                       relative from the fp64 one -- inside what F32J promises, not the DENSE_SCHUR digits. */

enum { SFMBA_PRECISION_F64  = 0,    /* everything fp64 (parity mode) */
       SFMBA_PRECISION_F32J = 1 };  /* fp32 Jacobian blocks AND fp32 observation coordinates (BASELINE config 3; the reference's
                                       observations are cv::Point2f anyway, BA.cpp:149-153 -- a caller holding genuinely double
                                       observations loses ~1e-4 px at 2k-px coordinates).  What is summed in which precision: a lane's OWN
                                       partial sum of block products is fp32 (at most 8 pair products of a 6x6 block of the reduced matrix,
                                       ceil(track / 4) point-block products of a point); every sum ACROSS lanes, chunks, points and ranks is
                                       fp64, and so are the residuals, the cost, the reduced system and its solve (ABI v4 summed a block's
                                       up-to-512 pair products in fp32 before widening).  The back-substitution evaluates the Jacobian-type terms of an observation (J x step,
                                       C = B~ L^-T) from an fp32 copy of the camera's R, t and step; the TRIAL residuals, which decide accept / reject, from the fp64 pose.
                                       The pair pass (the off-diagonal blocks of the reduced matrix), which forms no residual, evaluates the PROJECTION of
                                       its observations in fp32 as well, in both of its geometries (one wave or sixteen lanes per block).
                                       What to expect (tests/test_gpu_baseline_parity.py): final cost within 1e-6
                                       relative (measured 3e-13) and final RMS within 1e-4 px of the fp64 solve (measured < 1e-9 px),
                                       parameters within ~2e-5 -- EXCEPT points on weakly constrained tracks: a point seen by two
                                       nearly parallel views has almost no depth information, its 3x3 block is ill-conditioned and
                                       the fp32 rounding of its Jacobian moves it by up to ~1e-3..5e-3 scene units along the ray at
                                       (numerically) the same cost (cfg3_banded: 8e-4 and 2.1e-3 seen; the worst of 42 000 points of a 520-camera
                                       path: 0.03 .. 0.07, with 99.9 % of the points within 2e-3).  Use F64 if such points'
                                       coordinates matter beyond that. */

/* The F32J ERROR BUDGET (round 6): what SFMBA_PRECISION_F32J may cost against the library's fp64 mode under the same solver, in the units of the caller.
 * tests/test_gpu_f32j_budget.py measures every line on nine problem shapes, two solvers and two other scene scales (|t| ~ 1e3 and ~ 5e-2) and FAILS beyond
 * it: a faster fp32 kernel that moves a result past one of these numbers is a regression, not a tolerance to widen (rounds 4 - 5 loosened three tests to
 * make room for speed; this is where that stops).  scale = max(1, max |t|) of the solution: the budget does not depend on the units of the scene. */
/*                                             budget     measured, round 6 (profiles/r06_c_f32j_budget.txt: the worst of 22 runs)                          */
#define SFMBA_F32J_BUDGET_COST_REL     1e-8    /* 4.8e-10  final cost, relative (north_star asks 1e-6 at BASELINE config 2) */
#define SFMBA_F32J_BUDGET_RMS_PX       1e-6    /* 1.0e-10  final RMS reprojection error, px (north_star asks 1e-4) */
#define SFMBA_F32J_BUDGET_ROTATION     2e-5    /* 5.5e-6   angle-axis components of a camera, rad; LM iterations and termination type: identical */
#define SFMBA_F32J_BUDGET_TRANSLATION  1e-5    /* 1.6e-6   camera translation / scale */
#define SFMBA_F32J_BUDGET_FOCAL_REL    1e-6    /* 3.0e-9   the shared focal, relative */
#define SFMBA_F32J_BUDGET_POINT_P999   2e-5    /* 1.5e-6   99.9th percentile of the point displacement / scale (the weakly constrained tracks above are the rest) */
/* WHERE THE BUDGET DOES NOT APPLY (round 6, tests/fuzz_parity.py: 1 500 random shapes against the oracle; the fp64 modes follow it to <= 2e-8 of the
 * final cost on every one of them, over runs of up to 343 LM iterations).  F32J is for WELL-DETERMINED problems -- several observations per point, a few
 * hundred points per view, as every reconstruction the reference produces is.  On problems with about as many residuals as parameters (each point seen
 * twice, a handful of points for dozens of views) or dominated by gross outliers, the LM run takes tens of iterations, the trust region grows past ~1e7,
 * the damping falls below the rounding of the fp32 blocks and the reduced matrix stops being positive definite: steps become INVALID.  The library
 * then divides the radius by 8 instead of Ceres' 2 (F32J only; fp64 keeps the reference's rule) and goes on, and the run converges -- but to a final
 * cost that can differ from the fp64 one by 1e-4 .. 1e-3 relative, with a different iteration count, and not reproducibly from one run to the next (the
 * order in which fp64 atomics arrive is enough to tip an accept / reject decision on such a landscape; SFMBA_CREATE_DETERMINISTIC fixes the order).
 * Exactly satisfiable toy problems (final cost ~1e-8 of the initial one) end one LM iteration earlier or later than the oracle in F32J and with
 * the CG at 1e-8: both at a cost of zero for every purpose.  Use the default -- fp64 with SFMBA_LINEAR_AUTO -- when in doubt. */

/* Return codes of every entry point. */
enum {
    SFMBA_OK              = 0,
    SFMBA_ERR_INVALID_ARG = 1,
    SFMBA_ERR_NO_DEVICE   = 2,   /* HIP runtime/device missing: the product path never falls back to CPU */
    SFMBA_ERR_HIP         = 3,
    SFMBA_ERR_ALLOC       = 4,
    SFMBA_ERR_CAPACITY    = 5    /* an output array is too small: the required length was returned, nothing else written */
};

typedef struct sfmba_options {
    int    max_iters;                 /* 500    BA.cpp:174 */
    double max_seconds;               /* 10.0   BA.cpp:176; <= 0 disables the wall-clock limit */
    double function_tolerance;        /* 1e-6   Ceres default */
    double gradient_tolerance;        /* 1e-10  Ceres default */
    double parameter_tolerance;       /* 1e-8   Ceres default */
    double initial_radius;            /* 1e4    Ceres default initial_trust_region_radius */
    double max_radius;                /* 1e16 */
    double min_radius;                /* 1e-32 */
    double min_relative_decrease;     /* 1e-3 */
    double min_lm_diagonal;           /* 1e-6 */
    double max_lm_diagonal;           /* 1e32 */
    int    jacobi_scaling;            /* 1 */
    int    max_consecutive_invalid_steps; /* 5 */
    int    linear_solver;             /* SFMBA_LINEAR_* */
    int    precision;                 /* SFMBA_PRECISION_* */
    double pcg_tolerance;             /* CG residual tolerance (1e-8) */
    int    pcg_max_iters;             /* 0 = 4*dim */
    int    verbose;                   /* 0 silent (BA.cpp:177), 1 per-iteration lines on stderr */
    int    pcg_anchored;              /* 1: inside an LM solve the CG tolerance is anchored to the FIRST iteration's right-hand side,
                                         |r| <= tol * max(|b_k|, |b_first|), never looser than 1e-4 |b_k| -- every LM step is then solved
                                         to the same ABSOLUTE accuracy (pcg_common.h pcg_threshold_base).  0: plain relative residual. */
    /* ---- ABI v4: behaviour switches that were environment variables only (a C caller could not set them per problem or
       thread-safely).  0 = library default, 1 = on, -1 = off.  ABI v4 let the environment variable named beside each switch
       override the field; since ABI v5 NOTHING below sfmba_problem_create* reads the environment: the fields are the only way
       (what is still read from the environment, when a problem is BUILT: SFMBA_DETERMINISTIC, SFMBA_PAIR_LPB, SFMBA_PAIR_LOADS, SFMBA_PAIR_LIMIT,
       SFMBA_BUILD_TIMING; and per call of a front-end unit that works in groups the test hooks SFMBA_GROUP_BYTES and SFMBA_GROUP_ITEMS, which
       can only lower the scratch budget and the item cap of a group and never change an output). ---- */
    int    pcg_coarse_space;          /* SFMBA_PCG_COARSE         default on : two-level CG preconditioner (8 gauge vectors).  Where the reduced
                                         matrix is sparsely filled (< 1/2 of its blocks) with >= 90 % of the blocks within a quarter of the cyclic camera
                                         order -- views registered along a path -- and >= 32 cameras, the seven similarity vectors are used restricted to
                                         overlapping SEGMENTS of the camera order (eight up to 213 cameras, cameras / 25 <= 20 up to 1007: 3 - 15x fewer CG
                                         iterations there; AUTO keeps that CG above 213 cameras instead of factorising).
                                         1 = the eight global vectors only, 2 = the segments wherever they apply.
                                         The sharded solve keeps the eight global vectors (the choice would have to be agreed between the ranks). */
    int    pcg_symmetric;             /* ABI v6 (the slot ABI v4 called pcg_persistent; reserved in v5)  default on : the streaming CG (d > 1280, no
                                         segmented coarse space, not a deterministic handle) reads ONE triangle of S~ per iteration and uses every entry
                                         twice (k_sy_prod, pcg_symmetric.hip); the pair pass then writes that triangle only.  -1 = both triangles, the round-5 kernels */
    int    pcg_f32_matrix;            /* SFMBA_PCG_F32_MATRIX     default on : F32J + streaming CG (d > 1280) store S~ in fp32 */
    int    early_linearise;           /* SFMBA_EARLY_LINEARISE    default on : next linearisation enqueued before the host reads the verdict */
    int    shard_two_phase;           /* SFMBA_SHARD_TWO_PHASE    default on : sharded CG path exchanges (A) diagonal data, (B) preconditioned blocks */
    int    shard_f32_exchange;        /* SFMBA_SHARD_F32_EXCHANGE default on : exchange (B) in fp32 where the CG stores S~ in fp32 anyway */
    int    shard_distributed_cg;      /* SFMBA_SHARD_DIST_CG      default off: sharded CG path WITHOUT the redundant solve -- exchange (B) is a
                                         reduce-scatter of the upper-triangle blocks of S~ into ranges of block rows (half the bytes of the
                                         all-reduce), every rank multiplies the blocks it owns, one all-reduce of ld doubles per CG
                                         iteration's partial product (needs sfmba_problem_set_reduce_scatter when world > 1).
                                         2: the same CG with the product formed IMPLICITLY -- no pair pass, no
                                         exchange (B) at all: per CG iteration every rank applies its own points' W V^-1 W^T to the
                                         all-reduced vector (two passes over its observations) and the ranks all-reduce ld doubles
                                         (needs no reduce-scatter; duplicate (camera, point) observations are part of the implicit
                                         product: their cross terms are then NOT added to the diagonal blocks, which stay a preconditioner).
                                         3 (ABI v5; implied by a problem created with SFMBA_CREATE_ROW_SHARDED): block ROWS of S~ per rank.
                                         Every rank holds the whole problem; it eliminates its own range of points, the per-point table is
                                         ALL-GATHERED (88 bytes per point in F32J: 44 MB at 500k points), the camera-diagonal sums of the
                                         rank's share of the camera-major list go through exchange (A) as before, and the pair pass then
                                         forms the blocks of the rank's OWN block rows from ALL their pairs -- at one-GPU efficiency, no
                                         partial block ever crosses a rank, no exchange (B), no unpack.  The CG runs on the owned rows:
                                         per iteration one product launch, ONE all-reduce of ld + 16 (cameras / 4 + 1) doubles (the partial
                                         product and its partial dot products) and one update launch, all multi-workgroup. */
} sfmba_options;

/* Flags of sfmba_problem_create_ex (ABI v4; were environment variables read at create time). */
enum { SFMBA_CREATE_DETERMINISTIC = 1,    /* (SFMBA_DETERMINISTIC=1 in the environment forces it on) every workgroup owns its accumulator slot and multi-chunk
                                             sums are added in a fixed order, so results do not depend on the order fp64 atomics arrive in (bitwise reproducible
                                             run to run; ~30 % slower).  Sharded problems included (ABI v4), and the forms that apply the reduced matrix
                                             implicitly (shard_distributed_cg = 2, SFMBA_CREATE_NO_PAIR_LIST): the per-camera sums of a CG product are then
                                             written per chunk and added in chunk order (implicit_schur.hip).  The symmetric streaming CG (pcg_symmetric, ABI v6:
                                             its products arrive through atomics) is not used on such a handle. */
       SFMBA_CREATE_ROW_SHARDED = 2,      /* ABI v5, sfmba_problem_create_ex only: EVERY rank passes the WHOLE problem (all observations) with its rank / world;
                                             cam_active may be NULL.  The rank owns the points of a contiguous range of point slots (ceil(n / world) each), a
                                             contiguous share of the camera-major list and a balanced range of block rows of the reduced matrix
                                             (sfmba_options.shard_distributed_cg = 3).  Solved with sfmba_problem_solve_sharded (needs sfmba_problem_set_allgather
                                             when world > 1); always through the CG (SFMBA_LINEAR_CHOLESKY is treated as SFMBA_LINEAR_AUTO: CG to 1e-12).  After
                                             a solve every rank holds ALL parameters (the final points are all-gathered): sfmba_problem_get_params returns the
                                             whole solution on every rank. */
       SFMBA_CREATE_NO_PAIR_LIST = 4 };   /* ABI v5: do not build the list of observation pairs (4 bytes per pair of observations of one point: O(sum of squared
                                             track lengths) memory, and 2^31 pairs at most) and never form the reduced camera matrix: sfmba_problem_solve then runs the
                                             two-level CG with the matrix applied IMPLICITLY from the observations -- per CG iteration two passes over them, memory
                                             O(observations) whatever the track lengths.  A problem with 2^31 or more pairs (100 cameras that all see 440 000 points:
                                             the reference adds a residual block per (view, point) with no bound on the track length, BA.cpp:142-166) takes this path
                                             by itself -- no problem the reference's solver accepts is refused for its size.  Every linear_solver setting is served by
                                             that CG: SFMBA_LINEAR_PCG at pcg_tolerance, SFMBA_LINEAR_AUTO / _CHOLESKY at a relative residual of 1e-12 (the DENSE_SCHUR
                                             result to ~1e-10, not bit for bit); max_seconds is checked once per LM iteration; sfmba_problem_build_reduced and
                                             sfmba_problem_append are refused.  A resident handle that GROWS past 2^31 pairs in sfmba_problem_append takes this path
                                             from that append on (the append itself succeeds; the NEXT one is refused with SFMBA_ERR_INVALID_ARG "cannot grow in
                                             place" -- the drop-in shim then rebuilds).  Slower than the formed matrix wherever that fits (~8x per CG iteration at
                                             BASELINE config 5). */

typedef struct sfmba_summary {
    int    termination;               /* SFMBA_CONVERGENCE / NO_CONVERGENCE / FAILURE */
    int    iterations;                /* LM iterations taken (successful + unsuccessful) */
    int    successful_steps;
    int    unsuccessful_steps;
    int    residual_evals;            /* cost-only evaluations */
    int    jacobian_evals;            /* linearisations (residual + Jacobian) */
    int    linear_iters;              /* total PCG iterations (0 for Cholesky) */
    double initial_cost;
    double final_cost;
    double seconds;                   /* solve wall time, excludes H2D/D2H and structure build */
    double setup_seconds;             /* structure build + H2D (sfmba_solve only) */
    char   message[128];
    int    cholesky_fallbacks;        /* ABI v4: LM iterations of an AUTO solve whose CG did not reach 1e-12 and were factorised instead */
} sfmba_summary;

/* One row per LM iteration (row 0 = the initial evaluation), mirrors ceres::IterationSummary.  With x the point the iteration linearised at
 * and x_trial = x + step the point it tried (tests/test_gpu_trace_columns.py holds every column to a long-double restatement, row by row).
 * A row that ends the solve on a tolerance holds what Ceres had computed by then: the later columns are 0. */
typedef struct sfmba_iteration {
    int    iteration;
    int    step_is_valid;             /* the linear solve succeeded and the model cost change is positive; 0: the columns below it are 0, cost / gradient those of x */
    int    step_is_successful;        /* relative_decrease > min_relative_decrease: x_trial is the next x */
    int    linear_iters;              /* CG iterations of this row's linear solve (0: factorised) */
    double cost;                      /* at x_trial after a successful or a rejected step (Ceres reports the candidate's cost on a rejected row), else at x */
    double cost_change;               /* cost(x) - cost(x_trial) */
    double gradient_max_norm;         /* max |J^T r| over ALL parameters, unscaled, at the point the row leaves the solve at: x_trial after a successful
                                         step -- also when the iteration or time limit ends the solve with this row -- else the previous row's */
    double step_norm;                 /* |x_trial - x|_2 over cameras, points and the focal, unscaled: the difference of the stored parameters */
    double relative_decrease;         /* rho = cost_change / model cost change, the model's being -(J step)^T (r + J step / 2) with J, r at x */
    double trust_region_radius;       /* AFTER this row's update: radius / max(1/3, 1 - (2 rho - 1)^3) on success, radius / 2, 4, 8 ... on consecutive rejections */
} sfmba_iteration;

typedef struct sfmba_problem sfmba_problem;   /* opaque, device-resident problem */

SFMBA_API void        sfmba_options_default(sfmba_options* opt);
SFMBA_API int         sfmba_abi_version(void);
SFMBA_API const char* sfmba_last_error(void);
/* Number of visible HIP devices (0 if none / runtime missing). */
SFMBA_API int         sfmba_device_count(void);
/* Device memory of destroyed problems is kept in a bounded cache (<= 8 GB) and handed to the next problem, so that the
 * reference's call pattern -- adjustBundle() re-creating the problem after every added view, SfM.cpp:464-466 -- performs
 * no hipMalloc/hipFree in steady state.  This returns the cached memory to HIP; the number of bytes released. */
SFMBA_API long long   sfmba_release_cache(void);
/* ABI v6.  What the FIRST call of a process pays once -- the HIP context, the first pinned allocation, the first device chunks: 138 ms at BASELINE
 * config 3 against 2.6 - 3 ms for every later adjustBundle() -- can be paid at start-up instead: creates the context on `device`, one stream + pinned
 * block and device chunks for a problem of about `expected_obs` observations (0: the fixed-size pieces only) and leaves them in the cache the first
 * sfmba_problem_create* draws from.  Optional and idempotent; rc as everywhere (SFMBA_ERR_NO_DEVICE without a GPU). */
SFMBA_API int         sfmba_device_warmup(int device, int64_t expected_obs);

/*
 * One-shot solve == the ceres::Problem build + ceres::Solve of BA.cpp:109-179.
 * Parameters are updated in place for CONVERGENCE and NO_CONVERGENCE and left untouched for FAILURE (as Ceres
 * does); the shim applies the reference's "discard unless CONVERGENCE" rule (BA.cpp:182-185).
 * trace may be NULL; at most trace_cap rows are written and *trace_len receives the number written (with trace == NULL:
 * the number of rows the solve produced).
 */
SFMBA_API int sfmba_solve(int n_cam, double* cam6, int n_pt, double* pt3,
                int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                double* focal, const sfmba_options* opt, sfmba_summary* summary,
                sfmba_iteration* trace, int trace_cap, int* trace_len);

/*
 * Resident API: the problem (observation lists, structure, parameters) lives in HBM
 * across calls -- used by bench.py (inputs resident before the timed region) and by
 * the incremental caller (SfM.cpp:464-466 re-runs BA after every added view).
 */
SFMBA_API int  sfmba_problem_create(int device, int precision,
                          int n_cam, const double* cam6, int n_pt, const double* pt3,
                          int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                          double focal, sfmba_problem** out);
/* The same with create flags (SFMBA_CREATE_*); cam_active != NULL makes it a sharded problem exactly like
 * sfmba_problem_create_sharded (rank / world then matter; pass 0 / 1 otherwise). */
SFMBA_API int  sfmba_problem_create_ex(int device, int precision, int flags,
                          int n_cam, const double* cam6, const unsigned char* cam_active, int n_pt, const double* pt3,
                          int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                          double focal, int rank, int world, sfmba_problem** out);
/*
 * Grows a resident problem in place -- the incremental caller re-runs BA after every added view (SfM.cpp:464-466) with a
 * cloud that only ever GROWS (new points, new views of existing points, SfM.cpp:530-629): n_cam >= the previous n_cam and
 * n_pt >= the previous n_pt (new cameras / points at the END of the arrays), n_obs_new NEW observations (of old or new cameras
 * and points; indices into the full arrays).  The observations given before stay.  The parameters of ALL cameras and points
 * and the focal are replaced from cam6 / pt3 / focal (full arrays, as at create time): the caller's containers hold the
 * float-rounded result of the previous solve plus the new entries (BA.cpp:187-221).  The observation list never leaves the
 * device: the new observations are uploaded, merged into the point-major order by a device sort, and the dependent lists
 * (camera-major index, camera-pair lists, launch descriptors) are rebuilt on the device.  The problem solved afterwards is
 * the one sfmba_problem_create would build from the concatenated observation list (old observations first, then the new ones);
 * results agree with that up to floating-point reordering, NOT bit for bit: newly observed cameras / points take the next free
 * slot in order of first observation (create assigns slots in ascending caller index), so the reduced system is a symmetric
 * permutation of create's and sums are taken in a different order.
 * Slots are internal.  Every entry point speaks in caller indices, whatever the slots are: parameters and the point step of the
 * probe in the caller's arrays, per-observation outputs in the caller's observation order, and the reduced unknowns of
 * sfmba_problem_build_reduced (S, rhs, scale) and sfmba_problem_get_step_probe (z) with the ACTIVE cameras by ascending caller
 * index, six unknowns each, the focal last -- where the slots do not ascend (after an out-of-order append) those two test hooks
 * permute on the host on the way out; on a freshly created problem the device arrays go out as they are.
 * Failure contract: if the call fails after it has begun replacing the device structure (allocation or HIP error), the problem
 * is POISONED -- every later entry point on it returns SFMBA_ERR_INVALID_ARG ("poisoned") without touching the device and the
 * only valid call is sfmba_problem_destroy.  Argument errors (bad sizes, indices out of range) are detected first and leave the
 * problem as it was.
 */
SFMBA_API int  sfmba_problem_append(sfmba_problem* p, int n_cam, const double* cam6, int n_pt, const double* pt3,
                          int64_t n_obs_new, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy, double focal);
/* Restore the parameters given at create (or last append) time.  Nothing is enqueued by the call itself: the first kernel of the next
 * sfmba_problem_solve copies them on the device, and every other entry point that looks at the parameters does so first. */
SFMBA_API int  sfmba_problem_reset(sfmba_problem* p);
/* Overwrite the current parameters from host arrays (full-size arrays, as at create). */
SFMBA_API int  sfmba_problem_set_params(sfmba_problem* p, const double* cam6, const double* pt3, double focal);
SFMBA_API int  sfmba_problem_solve(sfmba_problem* p, const sfmba_options* opt, sfmba_summary* summary,
                         sfmba_iteration* trace, int trace_cap, int* trace_len);
SFMBA_API int  sfmba_problem_get_params(sfmba_problem* p, double* cam6, double* pt3, double* focal);
SFMBA_API void sfmba_problem_destroy(sfmba_problem* p);
/* The HIP stream all kernels of this problem are launched on (hipStream_t as void*). */
SFMBA_API void* sfmba_problem_stream(sfmba_problem* p);
/* Dimension of the reduced camera system: 6 * (#cameras with observations) + 1. */
SFMBA_API int  sfmba_problem_reduced_dim(const sfmba_problem* p);

/*
 * Per-kernel timing with HIP events recorded on the problem's own stream around every launch
 * (bench.py's `roofline` object).  set_profiling resets the counters.
 */
typedef struct sfmba_kernel_time {
    char    name[32];
    double  total_us;
    int64_t launches;
} sfmba_kernel_time;
SFMBA_API int sfmba_problem_set_profiling(sfmba_problem* p, int enable);
SFMBA_API int sfmba_problem_get_profile(sfmba_problem* p, sfmba_kernel_time* out, int cap, int* n);

/*
 * Step probe (a test hook, like sfmba_problem_build_reduced): what the LAST back-substitution that ran
 * on the handle consumed -- in any loop (sfmba_problem_solve, the matrix-free / sharded loop of
 * sfmba_problem_solve_sharded, sfmba_shard_solve_update).
 *   z   [dim]        the reduced step in build_reduced's unknowns (Jacobi-scaled, cameras in ascending
 *                    active order, focal last), after the block-Jacobi back-transform: the trial
 *                    cameras are x0 - scale * z.  NULL: not copied.
 *   dpt [3 * n_pt]   the point step k_point_update subtracted (unscaled, caller order; 0 for points
 *                    without observations): the trial points are x0 - dpt.  NULL: not copied.
 *   info             the reduced-system solver family that produced z, whether its CG read the matrix
 *                    in fp32, its coarse vectors (0, 8, 57 or 7 G + 1), the CG iterations of that LM
 *                    iteration, and whether AUTO fell back to the Cholesky on that linearisation.
 * Enabling it (re)arms the probe for the next solve: its buffers are allocated only while it is on, and
 * a solve with the probe off is the same solve.  get_step_probe waits for the problem's stream; family 0
 * means that no back-substitution has run since the probe was enabled.
 */
typedef struct sfmba_step_probe { int family; int f32_matrix; int coarse_vectors; int cg_iters; int cholesky_fallback; } sfmba_step_probe;
enum { SFMBA_FAMILY_CHOL_SMALL = 1, SFMBA_FAMILY_CHOL_FUSED, SFMBA_FAMILY_CHOL_PANEL, SFMBA_FAMILY_PCG_FAST, SFMBA_FAMILY_PCG_SEGMENTS,
       SFMBA_FAMILY_PCG_SYMMETRIC, SFMBA_FAMILY_PCG_STREAMING, SFMBA_FAMILY_PCG_SEGMENTS_STREAMING, SFMBA_FAMILY_PCG_SEGMENTS_STREAMING_SPARSE,
       SFMBA_FAMILY_DIST_BLOCKS, SFMBA_FAMILY_DIST_ROWS, SFMBA_FAMILY_IMPLICIT };
SFMBA_API int sfmba_problem_set_step_probe(sfmba_problem* p, int enable);
SFMBA_API int sfmba_problem_get_step_probe(sfmba_problem* p, double* z /*[dim]*/, double* dpt /*[3*n_pt] or NULL*/, sfmba_step_probe* info);

/*
 * Kernel-level entry points (parity tests call these through the C ABI).
 *   residuals_out : [2*n_obs] in the caller's observation order
 *   cost_out      : 1/2 sum r^2
 */
SFMBA_API int sfmba_problem_eval_residuals(sfmba_problem* p, double* residuals_out, double* cost_out);
/*
 * Jacobian blocks at the current parameters, UNSCALED, caller's observation order:
 *   jc [n_obs][2][6], jp [n_obs][2][3], jf [n_obs][2].  Any pointer may be NULL.
 */
SFMBA_API int sfmba_problem_eval_jacobian(sfmba_problem* p, double* jc, double* jp, double* jf);
/*
 * Damped, Jacobi-scaled reduced camera system at the current parameters for trust-region
 * radius `radius`:  S [dim*dim] row-major (symmetric, both triangles filled), rhs [dim],
 * scale [dim] = Jacobi column scaling of the reduced unknowns (cameras in ascending active
 * order, focal last).  jacobi_scaling follows opt (NULL = defaults).
 */
SFMBA_API int sfmba_problem_build_reduced(sfmba_problem* p, const sfmba_options* opt, double radius,
                                double* S, double* rhs, double* scale);
/* Dense SPD solve on the device (the reduced-system solver in isolation): A [n*n] row-major
 * symmetric, b [n] -> x [n].  method = SFMBA_LINEAR_*.  Returns SFMBA_OK and *info = 0 on success,
 * *info = k > 0 if the leading minor of order k is not positive definite. */
SFMBA_API int sfmba_dense_spd_solve(int device, int n, const double* A, const double* b, double* x,
                          int method, double pcg_tol, int pcg_max_iters, int* info, int* iters);
/* The reduced-system CG in isolation (a kernel-level hook for parity tests, like the one above): A [n*n] row-major symmetric positive
 * definite (the upper triangle is read), nrhs right-hand sides B [nrhs][n] solved one after another on ONE workspace -> X [nrhs][n] (the
 * solution in the unknowns of A, after the block-Jacobi back-transform).  The call sets what a handle sets per solve and then goes
 * through the library's own transform, path choice and family launches:
 *   Wt        [8][n] coarse vectors in the TRANSFORMED unknowns (x~ = Lb^T x, Lb = the Cholesky factors of the 6 x 6 diagonal blocks and
 *             the square root of a trailing scalar), fp32-representable values; NULL: no coarse space
 *             (with SFMBA_PCG_PROBE_SEGMENTS vectors 0 .. 6 must be zero at the trailing unknown, as the gauge vectors of a problem are)
 *   flags     SFMBA_PCG_PROBE_SYMMETRIC   the one-triangle streaming family where it applies (a non-deterministic handle's default)
 *             SFMBA_PCG_PROBE_F32_MATRIX  the transformed matrix is kept in fp32 where the family reads it so (n > 1280)
 *             SFMBA_PCG_PROBE_SEGMENTS    the segmented coarse space where it applies (needs Wt)
 *             SFMBA_PCG_PROBE_POISON      after the transform, NaN goes into everything the kernels promise not to multiply: columns >= n of
 *                                         the padded matrix and of the coarse vectors, the allocation slack behind both, and -- where the
 *                                         symmetric family runs -- the strict lower triangle
 *   tol       plain relative residual |r~| <= tol |b~| (not anchored)
 *   max_iters [nrhs], each in 1 .. 1000: solve i stops after max_iters[i] iterations at the latest and X[i] is the iterate it reached
 *   info      as sfmba_dense_spd_solve; iters [nrhs] or NULL: iterations per solve; path or NULL: family, f32_matrix, coarse_vectors of the
 *             last solve (cg_iters = its iterations).
 * A launch the runtime refuses is SFMBA_ERR_HIP at once; a size no family can launch is SFMBA_ERR_INVALID_ARG. */
enum { SFMBA_PCG_PROBE_SYMMETRIC = 1, SFMBA_PCG_PROBE_F32_MATRIX = 2, SFMBA_PCG_PROBE_SEGMENTS = 4, SFMBA_PCG_PROBE_POISON = 8 };
SFMBA_API int sfmba_dense_pcg_probe(int device, int n, const double* A, int nrhs, const double* B, const double* Wt, int flags, double tol,
                                    const int* max_iters, double* X, int* info, int* iters, sfmba_step_probe* path);
/* The distributed CG of the sharded forms (SFMBA_FAMILY_DIST_BLOCKS / SFMBA_FAMILY_DIST_ROWS) in isolation, every rank of a world of `world`
 * ranks simulated in THIS process on one device (a kernel-level hook for parity tests, like the one above; no communicator, no RCCL).
 * A [n*n] as above with n = 6 ncam + 1, B [nrhs][n] solved one after another on the same workspaces, Wt [8][n] as above or NULL.  The call
 * goes through the library's own transform, then gives every simulated rank k a workspace of its own (the library's partition of the block
 * rows, its own x, flags and info word) and that rank's chunk of the reduce-scatter layout: the upper off-diagonal 6 x 6 blocks of the
 * transformed matrix for the block rows rows[k] .. rows[k + 1].  Focal row, b~ and W~ are the buffers the sharded loop passes.  Every rank is
 * driven by the library's own set-up and iteration entry points; the all-reduce they call is an in-place sum over the ranks' buffers, added in
 * rank order, so every rank receives identical bits.
 *   flags     SFMBA_DCG_PROBE_F32     blocks AND focal row in fp32, together, as the sharded loop pairs them; only where the reduced matrix
 *                                     is stored in fp32 (n > 1280), SFMBA_ERR_INVALID_ARG elsewhere.  (The product kernels are also
 *                                     instantiated for fp32 blocks with an fp64 focal row and the reverse: no caller pairs them so, the
 *                                     mixed pairs are not reachable and not tested.)
 *             SFMBA_DCG_PROBE_POISON  NaN in the padding of every rank's chunk behind its last block, in columns >= n of the transformed
 *                                     matrix, of W~ and of b~: the kernels promise not to read these
 *   tol       plain relative residual |r~| <= tol |b~| (not anchored)
 *   max_iters [nrhs], each in 1 .. 1000: solve i is ended after max_iters[i] iteration launches at the latest (the done flag is then set
 *             as a converging launch sets it) and Xt[i] is the iterate it reached
 *   surplus   >= 0: that many further iteration launches per solve behind its end, each with its collective, as the fixed batches of the
 *             sharded loop issue them; they must change nothing
 *   Xt        [nrhs][n] rank 0's solution in the TRANSFORMED unknowns (x~ = Lb^T x)
 *   info      as sfmba_dense_spd_solve (the transform's, else rank 0's breakdown word); iters [nrhs] or NULL: iterations per solve
 *   rows      [world + 1] or NULL, chunk_blocks or NULL: the partition of the block rows and the blocks per chunk the library chose
 *   replicas_differ   or NULL: before every collective and at the end of every solve each rank's x, p, r (both parities), scalar state,
 *             thresholds, flags and info word are compared bit for bit with rank 0's on the device; 0, or the number of the first such
 *             check (counted from 1 over the whole call) that found a difference.
 * world outside 1 .. 16, n % 6 != 1, a max_iters entry outside 1 .. 1000 and unknown flags are SFMBA_ERR_INVALID_ARG before the device is
 * looked at. */
enum { SFMBA_DCG_PROBE_F32 = 1, SFMBA_DCG_PROBE_POISON = 2 };
SFMBA_API int sfmba_dist_cg_probe(int device, int n, const double* A, int world, int nrhs, const double* B, const double* Wt, int flags, double tol,
                                  const int* max_iters, int surplus, double* Xt, int* info, int* iters, int* rows, long long* chunk_blocks,
                                  int* replicas_differ);

/*
 * Sharded API (multi-GPU): every rank holds the observations of a disjoint set of points
 * and a replica of all cameras + the focal.  Points are independent given the cameras (the Schur
 * structure), so each rank eliminates its own points and the ONLY exchange per LM iteration is the
 * sum of the partial reduced camera systems:
 *
 *   begin -> [all-reduce SUM of setup_buf] -> setup_finish
 *   repeat: partial_build -> [all-reduce SUM of reduce_buf] -> solve_update
 *                         -> [all-reduce SUM of scalars_buf] -> finish(&done)
 *   end
 *
 * All buffers are DEVICE pointers owned by the problem (wrap them as torch tensors for
 * torch.distributed / RCCL); every phase is enqueued on sfmba_problem_stream().  Every rank solves the
 * reduced system redundantly and takes bit-identical accept/reject decisions (no broadcast).
 *   reduce_buf  = [ upper triangle of S, packed row after row (ld (ld + 1) / 2) | rhs (ld) | udiag (ld) | bc (ld) | scalars (SFMBA_SHARD_SCALARS) ]
 *   setup_buf   = [ udiag (ld) | bc (ld) | scalars ] of the problem's own system buffer (column norms for the Jacobi scaling, ||x||^2)
 *   scalars_buf = the last SFMBA_SHARD_SCALARS doubles (trial cost, model change, step norms; one
 *                 per-rank slot each for the gradient max-norm, gathered through the SUM)
 */
#define SFMBA_SHARD_SCALARS 80
SFMBA_API int     sfmba_problem_create_sharded(int device, int precision,
                          int n_cam, const double* cam6, const unsigned char* cam_active /* [n_cam] globally observed cameras */,
                          int n_pt, const double* pt3,
                          int64_t n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                          double focal, int rank, int world, sfmba_problem** out);
SFMBA_API int     sfmba_shard_begin(sfmba_problem* p, const sfmba_options* opt);
SFMBA_API int     sfmba_shard_setup_finish(sfmba_problem* p);
SFMBA_API int64_t sfmba_shard_reduce_len(const sfmba_problem* p);       /* doubles in reduce_buf */
SFMBA_API void*   sfmba_shard_reduce_buf(sfmba_problem* p);
SFMBA_API int64_t sfmba_shard_setup_len(const sfmba_problem* p);
SFMBA_API void*   sfmba_shard_setup_buf(sfmba_problem* p);
SFMBA_API void*   sfmba_shard_scalars_buf(sfmba_problem* p);            /* SFMBA_SHARD_SCALARS doubles */
SFMBA_API int     sfmba_shard_partial_build(sfmba_problem* p);          /* linearise own points: partial S / rhs / scalars */
SFMBA_API int     sfmba_shard_solve_update(sfmba_problem* p);           /* after all-reduce #1: solve, back-substitute, trial cost */
SFMBA_API int     sfmba_shard_finish(sfmba_problem* p, int* done);      /* after all-reduce #2: accept/reject, convergence */
SFMBA_API int     sfmba_shard_end(sfmba_problem* p, sfmba_summary* summary);

/*
 * The whole sharded LM loop in one call (the phase functions above remain for callers that drive the choreography themselves).
 * The all-reduces go through `allreduce(ctx, device_buf, n_doubles, hip_stream)` -- in-place SUM over the ranks, enqueued on
 * hip_stream, return 0 on success -- which may be NULL when world == 1.  Per LM iteration, exact solver: two (packed upper triangle
 * of S | rhs | diagonals | scalars, then 80 trial-step scalars).  CG solver: three -- (A) 6x6 diagonal blocks | camera-focal column
 * | rhs | diagonals | scalars, (B) the off-diagonal blocks of the block-Jacobi-PRECONDITIONED matrix (every rank transforms its
 * partial blocks with the factors that follow from (A): the transform is linear in S), (C) the 80 trial-step scalars.  Every rank
 * calls with the same options; what is decided from the reduced sums is then bit-identical on all of them.  sfmba_comm_* is the built-in one:
 * ncclAllReduce (RCCL, xGMI) bound with dlopen at first use; one communicator per rank, created from the 128-byte unique id
 * that rank 0 draws (sfmba_comm_unique_id) and the launcher distributes (bench.py: a torch.distributed broadcast).
 * The host meets the GPU once per LM iteration, at the control kernel's mailbox post; nothing is copied back inside the loop.
 * options.max_seconds is NOT applied in sharded solves (ranks would disagree on a wall clock); max_iters is.
 * Error behaviour is fail-stop, as with RCCL itself: every allocation the loop needs is made BEFORE the rank issues its first
 * collective, so a rank that cannot take part returns an error without having entered one; inside the loop only HIP / collective
 * errors remain.  A rank that returns an error leaves its peers blocked in their next collective: the caller must then tear the
 * job down -- sfmba_comm_abort (ncclCommAbort) on the built-in communicator makes the peers' pending collectives fail so that
 * they return SFMBA_ERR_HIP too.
 */
#define SFMBA_COMM_ID_BYTES 128
typedef struct sfmba_comm sfmba_comm;
typedef int (*sfmba_allreduce_fn)(void* ctx, void* device_buf, int64_t n_doubles, void* hip_stream);
SFMBA_API int  sfmba_comm_unique_id(unsigned char id[SFMBA_COMM_ID_BYTES]);
SFMBA_API int  sfmba_comm_create(const unsigned char id[SFMBA_COMM_ID_BYTES], int rank, int world, int device, sfmba_comm** out);
SFMBA_API void sfmba_comm_destroy(sfmba_comm* comm);
SFMBA_API int  sfmba_comm_size(const sfmba_comm* comm, int* world, int* rank);   /* ncclCommCount / ncclCommUserRank: what RCCL itself says the communicator is (bench.py's n_gpus) */
SFMBA_API int  sfmba_comm_abort(sfmba_comm* comm);      /* ncclCommAbort: call on the ranks that failed; the communicator is unusable afterwards */
SFMBA_API int  sfmba_comm_allreduce(void* comm /* sfmba_comm* */, void* device_buf, int64_t n_doubles, void* hip_stream);   /* an sfmba_allreduce_fn */
SFMBA_API int  sfmba_problem_solve_sharded(sfmba_problem* p, const sfmba_options* opt, sfmba_allreduce_fn allreduce, void* ctx,
                                 sfmba_summary* summary);
/* Optional single-precision all-reduce (same ctx as the fp64 one).  Where the CG stores the preconditioned matrix in fp32 anyway
 * (SFMBA_PRECISION_F32J and more than 1280 reduced unknowns: the streaming CG path) exchange (B) -- by far the largest: 18 Nc (Nc - 1)
 * values, 144 MB in fp64 at 1000 cameras -- is then summed and stored in fp32: half the bytes over xGMI, and the summed buffer is the
 * CG's matrix without a narrowing pass.  Without it (or with options.shard_f32_exchange = -1) every exchange stays fp64. */
typedef int (*sfmba_allreduce_f32_fn)(void* ctx, void* device_buf, int64_t n_floats, void* hip_stream);
SFMBA_API int  sfmba_comm_allreduce_f32(void* comm /* sfmba_comm* */, void* device_buf, int64_t n_floats, void* hip_stream);   /* an sfmba_allreduce_f32_fn */
SFMBA_API int  sfmba_problem_set_allreduce_f32(sfmba_problem* p, sfmba_allreduce_f32_fn allreduce_f32);                        /* NULL: fp64 only */
/* Collectives of the DISTRIBUTED CG (options.shard_distributed_cg, include above): exchange (B) becomes a reduce-scatter of the
 * upper-triangle blocks of S~ in a layout of `world` equal chunks (contiguous ranges of block rows, padded): after the call, stream-ordered,
 * recv_buf (= send_buf + rank * n_values elements: in place) holds the SUM over the ranks of chunk `rank`.  is_f32 != 0: the elements are
 * floats.  Every CG iteration then all-reduces ONE vector of ld doubles through the sfmba_allreduce_fn given to sfmba_problem_solve_sharded
 * (eight of them, in one call, at the coarse-space setup).  Without a reduce-scatter callback the option is ignored when world > 1. */
typedef int (*sfmba_reduce_scatter_fn)(void* ctx, void* send_buf, void* recv_buf, int64_t n_values, int is_f32, void* hip_stream);
SFMBA_API int  sfmba_comm_reduce_scatter(void* comm /* sfmba_comm* */, void* send_buf, void* recv_buf, int64_t n_values, int is_f32, void* hip_stream);   /* an sfmba_reduce_scatter_fn: ncclReduceScatter */
SFMBA_API int  sfmba_problem_set_reduce_scatter(sfmba_problem* p, sfmba_reduce_scatter_fn reduce_scatter);     /* NULL: none */
/* All-gather of the ROW-SHARDED solve (SFMBA_CREATE_ROW_SHARDED): in place -- buf holds `world` slices of bytes_per_rank bytes, slice `rank` is this
 * rank's contribution; after the call, stream-ordered, every slice holds its owner's bytes.  Called twice per linearisation (the two halves of the
 * per-point table) and once at the end of a solve (the final points). */
typedef int (*sfmba_allgather_fn)(void* ctx, void* buf, int64_t bytes_per_rank, void* hip_stream);
SFMBA_API int  sfmba_comm_allgather(void* comm /* sfmba_comm* */, void* buf, int64_t bytes_per_rank, void* hip_stream);   /* an sfmba_allgather_fn: ncclAllGather */
SFMBA_API int  sfmba_problem_set_allgather(sfmba_problem* p, sfmba_allgather_fn allgather);     /* NULL: none */
/* what the last sfmba_problem_solve_sharded() exchanged per linearisation: out = { bytes of (A), bytes of (B), bytes of (C), flags: bit 0 = (B) was fp32, bit 1 = distributed CG (then (B) = the bytes of the whole
 * reduce-scatter buffer, of which a rank receives 1 / world, and every CG iteration adds 8 ld bytes of all-reduce),
 * bit 2 = implicit Schur CG, bit 3 = row-sharded (then (B) = the bytes of the per-point table a rank RECEIVES through the all-gather) } */
SFMBA_API int  sfmba_shard_last_exchange(const sfmba_problem* p, int64_t out[4]);

/*
 * The step in front of bundle adjustment: SfMStereoUtilities::triangulateViews
 * (SfMToyLib/SfMStereoUtilities.cpp:120-206) for n ALIGNED matches -- normalise with K (no distortion), DLT
 * triangulation (cv::triangulatePoints), de-homogenise, re-project into both views; a match is kept unless an error >
 * max_reproj_px (the reference's MIN_REPROJECTION_ERROR = 10, :42; its test is norm(...) > 10, :186, so a NaN error is
 * kept), keep[i] = 1 then.  left_xy / right_xy [n][2] pixels, K [9]
 * row-major, P_left / P_right [12] row-major [R|t]; outputs points3d [n][3], keep [n] and (optional) reproj_err [n][2].
 * Host pointers; the computation runs on `device`.
 */
SFMBA_API int sfmba_triangulate(int device, int64_t n, const float* left_xy, const float* right_xy, const float* K,
                                const float* P_left, const float* P_right, float max_reproj_px,
                                float* points3d, unsigned char* keep, float* reproj_err);

/*
 * The same for the match lists of MANY pairs in one call -- the (good view, new view) pairs of one added view (SfM.cpp:413-444),
 * as sfmba_match_features / sfmba_essential_ransac hand them over: nothing is aligned on the host.
 *   img_ptr, pts, pair_left, pair_right, pair_ptr, query_idx, train_idx
 *                 exactly the arrays of sfmba_homography_ransac below (same checks, same refusals, left == right allowed).  Entry e of
 *                 pair p is the match pts[img_ptr[pair_left[p]] + query_idx[e]] -> pts[img_ptr[pair_right[p]] + train_idx[e]].
 *                 total = pair_ptr[n_pairs]; entries in front of pair_ptr[0] belong to no pair and are written as not kept.
 *   mask          [total] or NULL: the `inlier` array sfmba_essential_ransac returns.  An entry with mask == 0 gets keep = 0, a zero
 *                 point and zero errors, and is not listed.
 *   K [9], P_left / P_right [n_pairs][12], max_reproj_px (finite, >= 0)
 *                 as sfmba_triangulate takes them, one camera pair per pair.
 *   points3d [total][3], keep [total], reproj_err [total][2] or NULL
 *                 for every pair, byte for byte what sfmba_triangulate writes for that pair's aligned points and cameras.
 *   kept_ptr [n_pairs + 1], kept_idx [total]
 *                 kept_idx[kept_ptr[p] .. kept_ptr[p+1]-1] = the positions in the flattened list of the kept entries of pair p,
 *                 ascending; only the first kept_ptr[n_pairs] entries of kept_idx are defined.
 * Host pointers, synchronous.  SFMBA_ERR_INVALID_ARG (nothing written) for what sfmba_homography_ransac refuses, for a non-finite or
 * negative max_reproj_px and for 2^31 - 257 or more entries; n_pairs == 0 or no entry in any pair: SFMBA_OK, kept_ptr all zero.
 */
SFMBA_API int sfmba_triangulate_pairs(int device, int n_images, const int64_t* img_ptr, const float* pts /*[img_ptr[n_images]][2]*/,
                                      const float* K, int n_pairs, const int32_t* pair_left, const int32_t* pair_right,
                                      const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                                      const unsigned char* mask, const float* P_left, const float* P_right, float max_reproj_px,
                                      float* points3d, unsigned char* keep, float* reproj_err, int64_t* kept_ptr, int64_t* kept_idx);

/*
 * The two association loops of the incremental pipeline, results identical to the reference's loops
 * entry for entry and in the same order.
 *
 * Shared encodings
 *   cloud views   CSR over the cloud points: view_ptr [n_pt + 1]; entries view_idx / feat_idx = the point's originatingViews
 *                 (SfMCommon.h:87) in ASCENDING view index (std::map iteration order)
 *   match matrix  SfM::mFeatureMatchMatrix (SfM.h:50) flattened: pair p = [pair_left[p]][pair_right[p]], its cv::DMatch list is
 *                 entries pair_ptr[p] .. pair_ptr[p+1] of query_idx / train_idx (/ distance), in list order.  Only entries with
 *                 left <= right are ever consulted by the reference (SfM.cpp:489-490, 555-558); others are ignored here too.
 *
 * sfmba_find_2d3d_matches == SfM::find2D3DMatches (SfMToyLib/SfM.cpp:471-528): for every view v with view_done[v] == 0 and
 * every cloud point, the first originating view (ascending) that has a match to v for the point's feature -- the FIRST such
 * match in list order, matches whose other index is negative skipped (SfM.cpp:508) -- yields one entry
 * (cloud point index, feature index in view v).  Output: out_ptr [n_views + 1] (done views: empty ranges), entries in cloud
 * order inside a view; the reference's points2D / points3D are features[v].points[out_feature] / cloud[out_point].p.
 * *total receives the number of entries; SFMBA_ERR_CAPACITY (out_ptr and *total valid, nothing else written) if cap < *total.
 */
SFMBA_API int sfmba_find_2d3d_matches(int device, int n_views, const unsigned char* view_done,
                int n_pt, const int64_t* view_ptr, const int32_t* view_idx, const int32_t* feat_idx,
                int n_pairs, const int32_t* pair_left, const int32_t* pair_right, const int64_t* pair_ptr,
                const int32_t* query_idx, const int32_t* train_idx,
                int64_t* out_ptr, int32_t* out_point, int32_t* out_feature, int64_t cap, int64_t* total);
/*
 * The O(n^2) part of SfM::mergeNewPointCloud (SfMToyLib/SfM.cpp:538-544): which points of the cloud are closer than max_dist
 * (MERGE_CLOUD_POINT_MIN_MATCH_DISTANCE, SfM.cpp:50) to new point k.  "The cloud" as of new point k is the existing points
 * followed by the new points 0 .. k-1 that were appended before it (SfM.cpp:596-600), so the candidates of k are indices j of
 * the sequence [existing 0 .. n_exist-1, new 0 .. k-1] (j >= n_exist means new point j - n_exist) with
 * cv::norm(seq[j] - new[k]) < max_dist in the reference's arithmetic (float difference, double norm), ASCENDING -- the order
 * the reference's scan meets them in.  cand_ptr [n_new + 1], cand_idx [cap].  The sequential, data-dependent remainder of the
 * function (feature-match confirmation, views added to existing points) is host code: host/SfMAssociation.cpp.
 */
SFMBA_API int sfmba_merge_candidates(int device, int n_exist, const float* exist_xyz, int n_new, const float* new_xyz, float max_dist,
                int64_t* cand_ptr, int32_t* cand_idx, int64_t cap, int64_t* total);

/*
 * The feature match matrix (SfM::createFeatureMatchMatrix, SfMToyLib/SfM.cpp:157-212): SfM2DFeatureUtilities::matchFeatures
 * (SfM2DFeatureUtilities.cpp:53-71) -- a brute-force Hamming 2-NN and the ratio test -- for a list of image pairs in one call.
 *
 *   descriptors   image i owns rows img_ptr[i] .. img_ptr[i+1]-1 of desc; a row is desc_bytes bytes (1..64; ORB: 32), rows
 *                 packed back to back.  An image may hold at most 2^22 - 1 rows.
 *   pair p        query rows = the rows of image pair_left[p], train rows = those of image pair_right[p]; l == r is allowed.
 *   distance      d(q, j) = popcount(desc_l[q] XOR desc_r[j]) over the row's bytes (an integer <= 8 desc_bytes).
 *   2-NN          best(q), second(q) = the two smallest (d, j) in lexicographic order: a tie on distance goes to the lower
 *                 train index (OpenCV's BFMatcher::knnMatch, K = 2, inserts with a strict <).
 *   ratio test    q is kept iff the train image has >= 2 rows and (double)d_best < ratio * (double)d_second, in double as the
 *                 reference compares a float DMatch distance with NN_MATCH_RATIO.  The reference's value is ratio =
 *                 (double)0.8f = 0.800000011920929, with which d = 4 against 5 IS kept (an exact 0.8 would drop it).
 *                 The one deliberate departure: with fewer than 2 train rows the reference reads initialMatching[i][1] out of
 *                 bounds (undefined behaviour); here that pair has no matches.
 *   output        a kept query yields (query_idx = q, train_idx = j_best, distance = (float)d_best) -- the DMatch the reference
 *                 keeps (imgIdx = 0).  Entries are in ascending q within a pair (prunedMatching order), pairs in the order of
 *                 the pair list: pair_ptr [n_pairs + 1] is the CSR of the flattened match-matrix encoding that
 *                 sfmba_find_2d3d_matches reads.  An empty query or train image gives an empty list.  distance may be NULL.
 *
 * Host pointers in and out, synchronous.  *total receives the number of entries; SFMBA_ERR_CAPACITY (pair_ptr and *total valid,
 * nothing else written) if cap < *total.  SFMBA_ERR_INVALID_ARG for desc_bytes outside 1..64, an image with >= 2^22 rows, a pair
 * index out of range, a ratio that is not finite or <= 0, and more than 2^31 - 1 query rows (summed over the pairs) in one call.
 * Deterministic: the result does not depend on how the work is cut up.  The work is cut into batches of query tiles (512 query
 * rows of one pair) in pair-list order, at most 512 tiles per batch (a fixed 64 MiB bound on the per-slice scratch); a batch of
 * n tiles splits every train image into min(ceil(4096 / n), ceil(max train rows of the batch / 256), 32) slices (at least 1).
 */
SFMBA_API int sfmba_match_features(int device, int n_images, const int64_t* img_ptr, const unsigned char* desc, int desc_bytes,
                int n_pairs, const int32_t* pair_left, const int32_t* pair_right, double ratio,
                int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total);

/*
 * The same for FLOAT descriptors (SIFT, SURF, RootSIFT, learned ones): what cv::BFMatcher does with NORM_L2 -- an exact brute-force
 * L2 2-NN and the ratio test.  The encodings, the output order, the capacity protocol and the pair semantics are those of
 * sfmba_match_features; only these points differ:
 *
 *   rows          image i owns rows img_ptr[i] .. img_ptr[i+1]-1 of desc; a row is dims floats (1 <= dims <= 512), rows packed
 *                 back to back.  An image holds fewer than 2^22 rows.  Every value must be finite.
 *   s(q, j)       the squared distance, defined operation by operation: acc = 0.0f; for k = 0 .. dims-1 in ascending order
 *                 t = a[k] - b[k] (one fp32 subtraction), acc = fmaf(t, t, acc) (one fused fp32 operation); s = acc.  IEEE
 *                 behaviour throughout: subnormals are kept, nothing is flushed, nothing is reassociated.  From finite inputs s is
 *                 never NaN; it may be +inf.
 *   2-NN          the two smallest (s, j) in lexicographic order: a tie on s goes to the lower train index; +inf orders last.
 *   ratio test    dist = the correctly rounded fp32 square root of s.  q is kept iff the train image has >= 2 rows and
 *                 (double)dist_best < ratio * (double)dist_second.  So a best of +inf is dropped, a finite best against an
 *                 infinite second is kept, and two exact duplicates of the query (0 and 0) are dropped.
 *   output        (query_idx = q, train_idx = j_best, distance = dist_best).
 *
 * SFMBA_ERR_INVALID_ARG, before anything is written: dims outside 1..512, a non-finite value in desc (the message names the image
 * and the row), a ratio that is not finite or <= 0, an image with >= 2^22 rows, a pair index out of range, more than 2^31 - 1
 * query rows (summed over the pairs) in one call.  SFMBA_ERR_CAPACITY as for sfmba_match_features.
 * Deterministic: the result does not depend on how the work is cut up; no atomics, no arrival order.  The work is cut into batches
 * of query tiles (512 query rows of one pair) in pair-list order, at most 256 tiles per batch (a fixed 64 MiB bound on the
 * per-slice scratch, 16 bytes per query row and slice); a batch of n tiles splits every train image into
 * min(ceil(2048 / n), ceil(max train rows of the batch / 256), 32) slices (at least 1).  Inside a slice the train rows go through
 * LDS in stages of min(256, floor(8192 / dp / 16) * 16) rows, dp = dims rounded up to a multiple of 32, in groups of 16.
 */
SFMBA_API int sfmba_match_features_l2(int device, int n_images, const int64_t* img_ptr, const float* desc, int dims,
                int n_pairs, const int32_t* pair_left, const int32_t* pair_right, double ratio,
                int64_t* pair_ptr, int32_t* query_idx, int32_t* train_idx, float* distance, int64_t cap, int64_t* total);

/*
 * Pose a not-yet-registered view from its 2D-3D matches (SfMStereoUtilities::findCameraPoseFrom2D3DMatch,
 * SfMToyLib/SfMStereoUtilities.cpp:208-243: cv::solvePnPRansac + the inlier-ratio gate) for a batch of views in one call.
 * The reference's result depends on OpenCV's global RNG; THIS CONTRACT IS OUR OWN, deterministic one -- it is not, and does not
 * claim to be, the sample stream of cv::solvePnPRansac.
 *
 *   problems      problem p owns entries prob_ptr[p] .. prob_ptr[p+1]-1 of xyz [total][3] (world points) and uv [total][2]
 *                 (pixels); n = its number of entries.  With out_point / out_feature gathered this is the output of
 *                 sfmba_find_2d3d_matches (one problem per view).  K [9] row-major; only fx = K[0], fy = K[4], cx = K[2],
 *                 cy = K[5] are read.  There is no distortion (the reference's is all zeros, SfM.cpp:74).
 *   sample        mix(z) is splitmix64's output function: z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 *                 z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31 (all mod 2^64).  key = mix(seed + p); draw
 *                 k = 0, 1, .., 63 of hypothesis h is index mix(key ^ ((h << 8) | k)) mod n; the sample is the first four DISTINCT
 *                 indices in draw order; a hypothesis that has not found four by draw 63 is invalid.  Integer work: exact.
 *   hypothesis    unit bearings from ((u-cx)/fx, (v-cy)/fy, 1) in fp64; P3P on the first three correspondences (Grunert's
 *                 quartic solved in closed form, every real root polished by Newton, then the three distances polished by
 *                 Newton on the distance equations); of the solutions with positive depth at all four sample points the one
 *                 whose pixel error at the fourth point is smallest.  Invalid if there is none, or if two of the three 3D
 *                 points coincide.  An invalid hypothesis has hyp_count = -1 and a zero hyp_pose.
 *   score         a point is an inlier of a pose iff its depth is > 0 and its squared pixel reprojection error is
 *                 <= threshold_px^2.  One device function takes this decision for the count and for the mask (fp32 products
 *                 of the pose pre-multiplied by diag(fx, fy, 1) against the observation minus the principal point, division
 *                 free: decisions can differ from fp64 only within ~1e-3 px of the threshold), so
 *                 sum(inlier of p) == n_inliers == hyp_count[best_hypothesis] exactly.
 *   winner        the valid hypothesis with the largest count; ties go to the lowest h.  inlier [total] is the WINNER's mask
 *                 (as OpenCV returns the mask of the RANSAC model, not of the refined pose).  All n_hyp hypotheses are
 *                 evaluated: there is no confidence-based early stop.
 *   refine        Gauss-Newton in fp64 on the winner's inliers; residual = pixel reprojection; update R <- exp([dw]x) R,
 *                 t <- t + dt; stops when |(dw, dt)| < 1e-12 or after max_refine_iters steps (the shim passes 20; 0 = off).
 *                 Skipped when n_inliers < 4.  refine_iters = steps taken; refine_cost = 1/2 sum |r|^2 over the inliers at the
 *                 returned pose.
 *   status        0 ok | 1 fewer than 4 points: pose = [I|0], mask zero, best_hypothesis = -1 | 2 no valid hypothesis: same
 *                 outputs as 1 | 3 refinement met a non-finite value or a singular normal matrix: the unrefined winner is
 *                 returned (refine_iters = 0).
 *
 * Outputs: pose [n_prob][12] row-major [R|t] (fp64), inlier [total], result [n_prob]; optional (NULL or not) hyp_pose
 * [n_prob][n_hyp][12] and hyp_count [n_prob][n_hyp], every hypothesis' unrefined pose and inlier count.  Host pointers in and out,
 * synchronous.  A degenerate problem never makes the call fail: the others of the batch are still answered.
 * SFMBA_ERR_INVALID_ARG for n_hyp outside 1..65536, a non-finite or non-positive threshold_px, fx or fy, a negative or decreasing
 * prob_ptr, max_refine_iters < 0, a problem of 2^31 or more points.  Deterministic: the same arguments give the same bytes in
 * every output (counts are integer atomics; the normal equations are reduced in a fixed order).
 */
typedef struct sfmba_pnp_result { int status; int best_hypothesis; int n_inliers; int refine_iters; double refine_cost; } sfmba_pnp_result;
SFMBA_API int sfmba_pnp_ransac(int device, int n_prob, const int64_t* prob_ptr, const float* xyz, const float* uv, const float* K,
                int n_hyp, float threshold_px, uint64_t seed, int max_refine_iters,
                double* pose, unsigned char* inlier, sfmba_pnp_result* result, double* hyp_pose, int32_t* hyp_count);

/*
 * Rank the image pairs for the baseline (SfM::sortViewsForBaseline, SfMToyLib/SfM.cpp:333-364, through
 * SfMStereoUtilities::findHomographyInliers, SfMStereoUtilities.cpp:51-72: cv::findHomography(RANSAC, 10 px) + countNonZero(mask))
 * for a batch of image pairs in one call.  The reference's result depends on OpenCV's global RNG and on its confidence-based early
 * stop; THIS CONTRACT IS OUR OWN, deterministic one -- it is not, and does not claim to be, the sample stream of cv::findHomography.
 *
 *   problems      pair p owns entries pair_ptr[p] .. pair_ptr[p+1]-1 of query_idx / train_idx; n = its number of entries.  Entry i
 *                 is the correspondence x = pts[img_ptr[pair_left[p]] + query_idx[i]] -> x' = pts[img_ptr[pair_right[p]] +
 *                 train_idx[i]]; pts [img_ptr[n_images]][2] holds the key points of all images (pixels), image i owning rows
 *                 img_ptr[i] .. img_ptr[i+1]-1.  These are the arrays sfmba_match_features returns plus the key point
 *                 coordinates: the reference's GetAlignedPointsFromMatch is folded into the call and done on the device.
 *                 left == right and repeated indices inside a pair are allowed.
 *   sample        the stream of sfmba_pnp_ransac: key = mix(seed + p); draw k = 0, 1, .., 63 of hypothesis h is entry
 *                 mix(key ^ ((h << 8) | k)) mod n; the sample is the first four DISTINCT entries in draw order; a hypothesis
 *                 that has not found four by draw 63 is invalid.  Integer work: exact.
 *   hypothesis    fp64.  Each side's four points are normalised: their mean c is subtracted and the result divided by s, the
 *                 mean of |coordinate - c| over the eight numbers; s == 0 makes the hypothesis invalid.  With homogeneous
 *                 a_i = (x^_i, 1) and b_i = (x^'_i, 1) the four triple determinants dl_k = det[a_i a_j a_k] (triple k omits
 *                 point k and keeps ascending order) and dr_k likewise decide validity: invalid if any |dl_k| <= 1e-3 or any
 *                 |dr_k| <= 1e-3 (three of the four nearly collinear), and invalid if the four products dl_k dr_k do not all have
 *                 the same sign (the quad is not mapped with one orientation: some sample point would cross the line at
 *                 infinity).  Otherwise H is THE homography through the four correspondences (closed form: [b_0 b_1 b_2]
 *                 diag(mu_i / lambda_i) adj([a_0 a_1 a_2]) with lambda, mu the Cramer ratios of those determinants), de-normalised
 *                 and scaled so that its third row applied to (c_left, 1) is 1; w > 0 then holds at all four sample points.  An
 *                 invalid hypothesis has hyp_count = -1 and a zero hyp_H.
 *   score         a correspondence is an inlier of H iff w = h31 x + h32 y + h33 > 0 and |H x / w - x'|^2 <= threshold_px^2: the
 *                 forward transfer error only, which is what OpenCV's homography RANSAC scores.  One device function takes this
 *                 decision for the count and for the mask (fp32, division-free: (X, Y, W) = H (x, y, 1), W > 0 and
 *                 (X - x' W)^2 + (Y - y' W)^2 <= thr^2 W^2; decisions can differ from fp64 only within ~1e-3 px of the
 *                 threshold), so sum(inlier of p) == n_inliers == hyp_count[best_hypothesis] exactly.
 *   winner        the valid hypothesis with the largest count; ties go to the lowest h.  H [p] is the winner's hypothesis as it
 *                 stands: there is no least-squares refit (the reference's only consumer reads the mask count).  inlier is the
 *                 winner's mask.  All n_hyp hypotheses are evaluated: there is no confidence-based early stop.
 *   status        0 ok | 1 fewer than 4 matches: H = I, mask zero, best_hypothesis = -1, n_inliers = 0 | 2 no valid hypothesis:
 *                 same outputs as 1.  n_matches echoes the pair's number of entries.
 *
 * Outputs: H [n_pairs][9] row-major (fp64), inlier [pair_ptr[n_pairs]] (entries in front of pair_ptr[0] are written as 0), result
 * [n_pairs]; optional (NULL or not) hyp_H [n_pairs][n_hyp][9] and hyp_count [n_pairs][n_hyp], every hypothesis' H and inlier count.
 * Host pointers in and out, synchronous.  A degenerate pair never makes the call fail: the others of the batch are still answered.
 * SFMBA_ERR_INVALID_ARG for n_hyp outside 1..65536, a non-finite or non-positive threshold_px, a negative or decreasing img_ptr or
 * pair_ptr, a pair index out of range, a query_idx or train_idx outside its image (checked on the host before anything is launched),
 * a pair of 2^31 or more matches.  Deterministic: the same arguments give the same bytes in every output (counts are integer atomics).
 */
typedef struct sfmba_homography_result { int status; int best_hypothesis; int n_inliers; int n_matches; } sfmba_homography_result;
SFMBA_API int sfmba_homography_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts /*[img_ptr[n_images]][2]*/,
                int n_pairs, const int32_t* pair_left, const int32_t* pair_right,
                const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx,
                int n_hyp, float threshold_px, uint64_t seed,
                double* H /*[n_pairs][9]*/, unsigned char* inlier /*[pair_ptr[n_pairs]]*/, sfmba_homography_result* result,
                double* hyp_H /*[n_pairs][n_hyp][9] or NULL*/, int32_t* hyp_count /*[n_pairs][n_hyp] or NULL*/);

/*
 * Recover the relative pose of an image pair from its matches (SfMStereoUtilities::findCameraMatricesFromMatch,
 * SfMToyLib/SfMStereoUtilities.cpp:74-118: cv::findEssentialMat(RANSAC, 0.999, 1 px) + cv::recoverPose, Pleft = I, Pright = [R|t],
 * the matches pruned by the final mask) for a batch of image pairs in one call: the baseline loop (SfM.cpp:236-320) and the pairs
 * (good view, new view) of every added view (SfM.cpp:413-431).  The reference's result depends on OpenCV's global RNG and on its
 * confidence-based early stop; THIS CONTRACT IS OUR OWN, deterministic one -- it is not, and does not claim to be, the sample stream
 * of cv::findEssentialMat.  It is tested against a CPU restatement of itself (tests/essential_oracle.py).
 *
 *   problems      the arrays of sfmba_homography_ransac (n_images, img_ptr, pts, n_pairs, pair_left, pair_right, pair_ptr, query_idx,
 *                 train_idx: entry i of pair p is x = pts[img_ptr[pair_left[p]] + query_idx[i]] -> x' = pts[img_ptr[pair_right[p]] +
 *                 train_idx[i]], gathered on the device) plus K [9] row-major, of which only fx = K[0], fy = K[4], cx = K[2],
 *                 cy = K[5] are read, as in sfmba_pnp_ransac.  left == right and repeated indices inside a pair are allowed.
 *   sample        the stream of sfmba_pnp_ransac: key = mix(seed + p); draw k = 0, 1, .., 63 of hypothesis h is entry
 *                 mix(key ^ ((h << 8) | k)) mod n; the sample is the first SIX DISTINCT entries in draw order; a hypothesis that
 *                 has not found six by draw 63 is invalid.  Entries 0..4 go to the solver, entry 5 selects among its solutions.
 *                 Integer work: exact.
 *   hypothesis    fp64, on the normalised points x = ((u - cx) / fx, (v - cy) / fy, 1).  The four-dimensional null space of the
 *                 5 x 9 epipolar system x'^T E x = 0 (invalid if the system is rank-deficient: a pivot of the completely pivoted
 *                 elimination at or below 1e-12 of its largest entry -- five collinear or coinciding points); the ten cubic
 *                 constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 on the 20 monomials of (x, y, z) up to degree 3;
 *                 elimination of the 10 x 20 system (invalid if the eliminated 10 x 10 block is singular: a pivot at or below 1e-13
 *                 of the largest entry); the real solutions -- at most 10 -- from the real roots of the degree-10 polynomial in z
 *                 (Sturm's sequence and bisection, two Newton steps), x and y back-substituted, each solution then polished by three
 *                 Gauss-Newton steps on the ten constraints themselves.  Every solution is scaled to Frobenius norm sqrt 2; of them
 *                 the one with the smallest squared Sampson distance at the sixth correspondence (normalised points; the first in
 *                 ascending z on a tie) is kept and its sign fixed so that its entry of largest magnitude (the first on ties, row-
 *                 major) is positive.  Invalid if there is no real solution or on any non-finite value.  An invalid hypothesis has
 *                 hyp_count = -1 and a zero hyp_E.  hyp_nsol = the number of real solutions found.
 *   score         the squared Sampson distance in pixels, cv::findEssentialMat's error: with centred pixels p = (u - cx, v - cy, 1),
 *                 F = diag(1/fx, 1/fy, 1) E diag(1/fx, 1/fy, 1), l' = F p, l = F^T p' and e = p' . l', a correspondence is an inlier
 *                 iff e^2 <= threshold_px^2 (l'_1^2 + l'_2^2 + l_1^2 + l_2^2) and that sum is > 0.  One device function takes this
 *                 decision for the count and for the mask (division-free on centred pixels, F scaled by fx fy; the residual e in
 *                 fp64, because its terms cancel from ~fx fy down to a pixel and the fp32 bound of that leaves the 5e-3 px band; the
 *                 gradient sum in fp32: decisions can differ from fp64 only within ~1e-6 px of the threshold), so
 *                 n_inliers == hyp_count[best_hypothesis] == the size of the winner's mask exactly.
 *   winner        the valid hypothesis with the largest count; ties go to the lowest h.  E [p] is the winner's hypothesis as it
 *                 stands: there is no refit.  All n_hyp hypotheses are evaluated: there is no confidence-based early stop.
 *   pose          recoverPose in fp64 on the winner's inliers only.  The four candidates in closed form (Horn 1990): t t^T =
 *                 1/2 tr(E E^T) I - E E^T, t = its column with the largest diagonal entry (the first on ties) over the root of that
 *                 entry, so |t| = 1; R(+-t) = cof(E) - [+-t]x E with cof the cofactor matrix (not its transpose).  Candidate order:
 *                 (R(+t), +t), (R(-t), -t), (R(-t), +t), (R(+t), -t).  An inlier is IN FRONT for a candidate iff the least-squares
 *                 depths lambda, lambda' of lambda' x' = lambda R x + t satisfy 0 < lambda < 50 and 0 < lambda' < 50 and the
 *                 determinant of their 2 x 2 normal equations, |R x  x  x'|^2, is > 0 (50 is OpenCV's distanceThresh at |t| = 1).
 *                 The pose is the candidate with the most points in front, ties to the lowest index (integer counts).  inlier is
 *                 the winner's mask AND in-front-for-the-chosen-pose, as recoverPose updates its mask and the reference prunes.
 *   status        0 ok | 1 fewer than 6 matches: E = 0, pose = [I|0], mask zero, best_hypothesis = -1, n_inliers = 0 | 2 no valid
 *                 hypothesis: same outputs as 1 | 3 a winner, but no point in front for any candidate (or E has no translation):
 *                 E, best_hypothesis and n_inliers are valid, pose = [I|0], mask zero.  n_pose_inliers = the size of the final mask;
 *                 pose_candidate = 0..3, -1 unless status is 0; n_matches echoes the pair's number of entries.
 *
 * Outputs: E [n_pairs][9] row-major (fp64), pose [n_pairs][12] row-major [R|t] (fp64), inlier [pair_ptr[n_pairs]] (entries in front
 * of pair_ptr[0] are written as 0), result [n_pairs]; optional (NULL or not) hyp_E [n_pairs][n_hyp][9], hyp_count [n_pairs][n_hyp]
 * and hyp_nsol [n_pairs][n_hyp].  Host pointers in and out, synchronous.  A degenerate pair never makes the call fail: the others of
 * the batch are still answered.  SFMBA_ERR_INVALID_ARG for n_hyp outside 1..65536, a non-finite or non-positive threshold_px, fx or
 * fy, a negative or decreasing img_ptr or pair_ptr, a pair index out of range, a query_idx or train_idx outside its image (checked on
 * the host before anything is launched), a pair of 2^31 or more matches.  Deterministic: the same arguments give the same bytes in
 * every output (counts are integer atomics).
 */
typedef struct sfmba_essential_result { int status; int best_hypothesis; int n_inliers; int n_pose_inliers; int pose_candidate; int n_matches; } sfmba_essential_result;
SFMBA_API int sfmba_essential_ransac(int device, int n_images, const int64_t* img_ptr, const float* pts /*[img_ptr[n_images]][2]*/,
                int n_pairs, const int32_t* pair_left, const int32_t* pair_right,
                const int64_t* pair_ptr, const int32_t* query_idx, const int32_t* train_idx, const float* K /*[9]*/,
                int n_hyp, float threshold_px, uint64_t seed,
                double* E /*[n_pairs][9]*/, double* pose /*[n_pairs][12]*/, unsigned char* inlier /*[pair_ptr[n_pairs]]*/,
                sfmba_essential_result* result, double* hyp_E /*[n_pairs][n_hyp][9] or NULL*/,
                int32_t* hyp_count /*[n_pairs][n_hyp] or NULL*/, int32_t* hyp_nsol /*[n_pairs][n_hyp] or NULL*/);

/*
 * Extract the features of a batch of images (SfM::extractFeatures, SfMToyLib/SfM.cpp:141-154: SfM2DFeatureUtilities::extractFeatures,
 * SfM2DFeatureUtilities.cpp:46-51, i.e. ORB::create(5000)->detectAndCompute per image) in one call: an ORB-style detector and a
 * steered-BRIEF descriptor of 32 bytes.  OpenCV's learned 256-pair table is not reproduced; THIS CONTRACT IS OUR OWN, deterministic
 * one -- it is not, and does not claim to be, cv::ORB.  It is integer arithmetic end to end (the three places that use double say
 * so), so the device is held BIT FOR BIT to a CPU restatement of itself (tests/orb_oracle.py).  Departures from cv::ORB: our own
 * pattern (steered BRIEF, not the learned rBRIEF table); 30 orientation bins; Harris ranks ALL non-maximum-suppressed FAST corners
 * (no pre-cut by FAST score); fixed-point resampling and smoothing; no mask.
 *
 *   images        image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of pixels: height[i] rows of width[i] * channels bytes, rows tight.
 *   gray          channels == 3 (B, G, R): g = (1868 B + 9617 G + 4899 R + 8192) >> 14.  channels == 1: the byte as it is.
 *   pyramid       in double: s_0 = 1, s_l = s_{l-1} * (double)scale_factor.  Level l is w_l = floor(w / s_l + 0.5) wide, h_l likewise,
 *                 and is resampled from level l - 1 (not from level 0).  Per axis, for destination index d, source length n and
 *                 destination length m: num = (2 d + 1) n - m, den = 2 m, i0 = num / den, f = ((num - i0 den) 2048 + den / 2) / den,
 *                 i1 = min(i0 + 1, n - 1).  The value is ((I00 (2048 - fx) + I01 fx) (2048 - fy) + (I10 (2048 - fx) + I11 fx) fy + 2^21)
 *                 >> 22.  A level with w_l <= 62 or h_l <= 62 has no key points; a level of size 0 ends the pyramid.
 *   FAST score    the 16-pixel circle of radius 3, clockwise from (0,-3): (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3)
 *                 (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).  d_k = c_k - p (circle pixel k, centre p);
 *                 S = max over the 16 starts s of max(min_{k<9} d_{s+k}, min_{k<9} -d_{s+k}), indices mod 16; S <= fast_threshold
 *                 counts as 0.  S is defined for pixels at least 3 from every edge.
 *   candidates    a pixel is a candidate iff S > 0, S is strictly greater than S at each of its 8 neighbours, and it lies at least
 *                 31 from every edge of its level.  Equal neighbours drop each other, as OpenCV's non-maximum suppression does.
 *   response      exact int64.  3 x 3 Sobel: Ix = (I[y-1][x+1] + 2 I[y][x+1] + I[y+1][x+1]) - (I[y-1][x-1] + 2 I[y][x-1] + I[y+1][x-1]),
 *                 Iy likewise with rows and columns exchanged; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 block centred
 *                 on the candidate; R = 25 (a b - c^2) - (a + b)^2 (Harris with k = 0.04, scaled by 25).  a, b <= 5.1e7, so 25 a b
 *                 stays below 2^63.
 *   quota         in double: f = 1 / (double)scale_factor, f^n_levels by repeated multiplication, want_0 = n_features (1 - f) /
 *                 (1 - f^n_levels); q_l = rint(want_l) (round-half-even), want_{l+1} = want_l f; the last level gets
 *                 max(n_features - sum, 0).  (5000, 1.2, 8) gives 1086 905 754 628 524 436 364 303.  A level with fewer candidates
 *                 than its quota keeps them all; nothing is redistributed.
 *   selection     a level keeps its first q_l candidates in the total order (R descending, then y ascending, then x ascending); that
 *                 is also the output order within a level; levels are ascending within an image.
 *   orientation   m10 = sum u I(x+u, y+v), m01 = sum v I(x+u, y+v) over the unblurred level and the disc u^2 + v^2 <= 225.  The bin
 *                 is the lowest k in 0..29 that maximises m10 C_k + m01 S_k in int64, with C_k = floor(16384 cos(2 pi k / 30) + 0.5):
 *                   16384 16026 14968 13255 10963 8192 5063 1713 -1713 -5063 -8192 -10963 -13255 -14968 -16026
 *                   -16384 -16026 -14968 -13255 -10963 -8192 -5063 -1713 1713 5063 8192 10963 13255 14968 16026
 *                 and S_k = floor(16384 sin(2 pi k / 30) + 0.5):
 *                   0 3406 6664 9630 12176 14189 15582 16294 16294 15582 14189 12176 9630 6664 3406
 *                   0 -3406 -6664 -9630 -12176 -14189 -15582 -16294 -16294 -15582 -14189 -12176 -9630 -6664 -3406
 *                 (the 12-degree discretisation of the ORB paper; no atan2, so nothing can differ in the last bit).
 *   smoothing     the separable 7-tap filter [18 34 49 54 49 34 18] (sum 256): horizontal pass, vertical pass, then (v + 32768) >> 16.
 *                 Defined for pixels at least 3 from every edge; nothing nearer an edge is ever read (the pattern reaches 13, and
 *                 13 + 3 < 31).
 *   pattern       mix = splitmix64's output function (sfmba_pnp_ransac).  A coordinate is mix(k) % 13 + mix(k+1) % 13 - 12 with k
 *                 advancing by 2 from 0; a pair takes four coordinates x0 y0 x1 y1 and is skipped if either point has x^2 + y^2 > 169
 *                 or the two points coincide; the first 256 accepted pairs form the pattern.  Rotation into bin k:
 *                 x' = (C_k x - S_k y + 8192) >> 14, y' = (S_k x + C_k y + 8192) >> 14 (arithmetic shift); every rotated point has
 *                 |x'|, |y'| <= 13.
 *   descriptor    bit i = 1 iff B(x + x0', y + y0') < B(x + x1', y + y1') with B the smoothed level; bit i is bit i % 8 of byte i / 8.
 *   key point     x = (float)(x_l * s_l) and y likewise (one double multiply each), size = (float)(31 s_l), angle = 12 bin degrees,
 *                 response = (float)R, octave = l.
 *
 * Outputs: kp_ptr [n_images + 1], kp [cap], desc [cap][32]; desc and kp_ptr go into sfmba_match_features as they come (as desc /
 * img_ptr with desc_bytes = 32).  Optional (NULL or not): dbg_level_xy [cap][2] = (x_l, y_l), dbg_bin [cap], dbg_harris [cap] = R,
 * dbg_candidates [n_images][n_levels] = the number of candidates of every level.  Host pointers in and out, synchronous.
 * *total receives the number of key points; SFMBA_ERR_CAPACITY (kp_ptr and *total valid, nothing else written) if cap < *total;
 * cap >= n_images * n_features always suffices.  SFMBA_ERR_INVALID_ARG for channels other than 1 or 3, a dimension outside 1..16384,
 * an img_ptr that does not agree with the sizes, n_features < 1, n_levels outside 1..12, a scale_factor that is not finite or lies
 * outside (1, 2], a fast_threshold outside 1..254.  Deterministic: the result does not depend on how the work is cut up (images go to
 * the device in consecutive groups under a fixed scratch bound); a batch equals the concatenation of single-image calls.
 * SFMBA_ABI_VERSION stays 6: adding a symbol is backward compatible.
 */
typedef struct sfmba_orb_keypoint { float x, y, size, angle, response; int32_t octave; } sfmba_orb_keypoint;
SFMBA_API int sfmba_orb_extract(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                int n_features, float scale_factor, int n_levels, int fast_threshold,
                int64_t* kp_ptr /*[n_images+1]*/, sfmba_orb_keypoint* kp, unsigned char* desc /*[cap][32]*/, int64_t cap, int64_t* total,
                int32_t* dbg_level_xy /*[cap][2] or NULL*/, int32_t* dbg_bin /*[cap] or NULL*/, int64_t* dbg_harris /*[cap] or NULL*/,
                int32_t* dbg_candidates /*[n_images][n_levels] or NULL*/);

/*
 * Extract FLOAT descriptors of a batch of images in one call: a Fast-Hessian detector and a SURF-style descriptor of 64 floats, the
 * extractor that goes with sfmba_match_features_l2 (the reference's lineage ran SURF_GPU in front of BruteForceMatcher_GPU<L2<float>>,
 * legacy/SfMToyLib_Old/GPUSURFFeatureMatcher.cpp:56).  THIS CONTRACT IS OUR OWN -- it is not, and does not claim to be,
 * cv::xfeatures2d::SURF.  Everything up to the final normalisation is box sums over an integral image of 8-bit pixels, exact integer
 * arithmetic, so the device is held BIT FOR BIT to a CPU restatement of itself (tests/surf_oracle.py).  Departures from SURF: no
 * sub-pixel or sub-scale interpolation of the extremum, one Gaussian over the whole descriptor window, orientation from the weighted
 * resultant of the Haar responses in 30 bins.  Match quality under rotation and scale is reported (README), not guaranteed.
 *
 *   images        as sfmba_orb_extract: image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of pixels, rows tight; the same gray rule.
 *   box sum       Box(y0, x0, h, w) = the sum of the gray values over rows y0 .. y0+h-1 and columns x0 .. x0+w-1, pixels outside the
 *                 image counting 0: the four coordinates are clamped into [0, height] x [0, width] of the integral image, and nothing
 *                 outside the integral image is ever read.  The integral image is kept mod 2^32; every box used is below 2^32.
 *                 All integer quantities below are int64 unless stated otherwise.
 *   layers        octave o (0-based) has four filter sizes L = 3 (2^(o+1) (i + 1) + 1), i = 0..3: 9 15 21 27 / 15 27 39 51 /
 *                 27 51 75 99 / 51 99 147 195.  Lobe l = L / 3, b = (L - 1) / 2.  Grid step s = 2^o, positions x = s i, y = s j inside
 *                 the image.
 *   responses     Dyy = Box(y-b, x-l+1, L, 2l-1) - 3 Box(y-(l-1)/2, x-l+1, l, 2l-1),
 *                 Dxx = Box(y-l+1, x-b, 2l-1, L) - 3 Box(y-l+1, x-(l-1)/2, 2l-1, l),
 *                 Dxy = Box(y-l, x+1, l, l) + Box(y+1, x-l, l, l) - Box(y-l, x-l, l, l) - Box(y+1, x+1, l, l),
 *                 N = 100 Dxx Dyy - 81 Dxy^2 (|N| < 2^53), H = (double)N / (double)(100 L^4): one IEEE division, the only
 *                 floating-point operation of the detector.  laplacian = (Dxx + Dyy >= 0) ? 1 : -1.
 *   candidates    the middle layers m = 1, 2 of every octave are searched.  With bt = (L_{m+1} - 1) / 2, a grid position is a
 *                 candidate iff x - s - bt >= 0, x + s + bt <= width - 1 and likewise in y (none of the 27 filters involved is clipped;
 *                 an image narrower or lower than 24 has no key points), H > (double)hessian_threshold, and H is strictly greater than
 *                 all 26 neighbours: grid steps +-s in the layers m-1, m, m+1 of the same octave.  Equal neighbours drop each other.
 *   selection     per image the first n_features candidates in the total order (H descending, then octave, layer, y, x ascending);
 *                 that is also the output order.
 *   Haar          HaarX(y, x, p) = Box(y-p, x, 2p, p) - Box(y-p, x-p, 2p, p), HaarY(y, x, p) = Box(y, x-p, p, 2p) - Box(y-p, x-p, p, 2p).
 *                 The scale sigma = 0.4 l is held as a rational: r = floor((4 l + 5) / 10), rnd(i) = floor((4 l i + 5) / 10), floor
 *                 division throughout, also for negatives.
 *   orientation   (upright == 0) over integer (i, j) with i^2 + j^2 < 36 (109 samples): mx += Wg(i,j) HaarX(y + rnd(j), x + rnd(i), 2r),
 *                 my likewise with HaarY.  Wg(i,j) = floor(65536 exp(-(i^2 + j^2) / 12.5) + 0.5), as [|j|][|i|] for 0..5:
 *                   65536 60497 47589 31900 18221 8869 / 60497 55846 43930 29447 16821 8187 / 47589 43930 34557 23164 13231 6440 /
 *                   31900 29447 23164 15527 8869 4317 / 18221 16821 13231 8869 5066 2466 / 8869 8187 6440 4317 2466 1200
 *                 The bin is the lowest k in 0..29 that maximises mx C_k + my S_k with the C_k, S_k of sfmba_orb_extract.
 *                 upright == 1: bin 0, moments reported as 0.
 *   descriptor    with C, S of the bin and d = 5 * 16384, for i, j in -10..9, a = 2i + 1, b = 2j + 1:
 *                 ox = floor((2 l (C a - S b) + d) / (2d)), oy = floor((2 l (S a + C b) + d) / (2d)); hx, hy = HaarX / HaarY(y + oy,
 *                 x + ox, r); dx = C hx + S hy, dy = -S hx + C hy; w = Wd(a,b) = floor(4096 exp(-(a^2 + b^2) / 87.12) + 0.5), as
 *                 [(|b|-1)/2][(|a|-1)/2] for |a|, |b| = 1, 3, .. 19:
 *                   4003 3652 3039 2307 1598 1010 582 306 147 64 / 3652 3331 2772 2105 1458 921 531 279 134 59 /
 *                   3039 2772 2307 1752 1213 767 442 232 111 49 / 2307 2105 1752 1330 921 582 335 176 85 37 /
 *                   1598 1458 1213 921 638 403 232 122 59 26 / 1010 921 767 582 403 255 147 77 37 16 /
 *                   582 531 442 335 232 147 85 44 21 9 / 306 279 232 176 122 77 44 23 11 5 /
 *                   147 134 111 85 59 37 21 11 5 2 / 64 59 49 37 26 16 9 5 2 1
 *                 Sub-region p = floor((i + 10) / 5), q = floor((j + 10) / 5), base = (4q + p) 4: v[base] += w dx, v[base+1] += w dy,
 *                 v[base+2] += w |dx|, v[base+3] += w |dy|.  Every |v| stays below 2^53 for n_octaves <= 4 (bound 4.8e14).
 *   normalisation M = max |v|, sh = max(0, bitlength(M) - 23), t_d = v_d >> sh (arithmetic shift), n2 = sum t_d^2 (exact, below 2^52),
 *                 desc_d = (float)((double)t_d / sqrt((double)n2)): a correctly rounded double square root, one double division, one
 *                 rounding to float.  n2 == 0 gives 64 zeros.  No step has a multiply followed by an add.
 *   key point     x = (float)x, y = (float)y, size = (float)L, angle = 12 bin degrees, response = (float)H, octave = o, layer = m,
 *                 laplacian as above.
 *
 * Outputs: kp_ptr [n_images + 1], kp [cap], desc [cap][64]; desc and kp_ptr go into sfmba_match_features_l2 as they come (as desc /
 * img_ptr with dims = 64).  Optional (NULL or not): dbg_bin [cap], dbg_moments [cap][2] = (mx, my), dbg_sums [cap][64] = v,
 * dbg_candidates [n_images][n_octaves][2] = the number of candidates of layers 1 and 2 of every octave before the cut.  Host pointers
 * in and out, synchronous.  *total receives the number of key points; SFMBA_ERR_CAPACITY (kp_ptr and *total valid, nothing else
 * written) if cap < *total; cap >= n_images * n_features always suffices.  SFMBA_ERR_INVALID_ARG (nothing written) for whatever
 * sfmba_orb_extract refuses about images, n_features < 1, n_octaves outside 1..4, a hessian_threshold that is not finite or is
 * negative, upright other than 0 or 1.  Deterministic: the same arguments give the same bytes, the result does not depend on how the
 * work is cut up (images go to the device in consecutive groups under a fixed scratch bound); a batch equals the concatenation of
 * single-image calls.  SFMBA_ABI_VERSION stays as it is: adding a symbol is backward compatible.
 */
typedef struct sfmba_surf_keypoint { float x, y, size, angle, response; int32_t octave, layer, laplacian; } sfmba_surf_keypoint;
SFMBA_API int sfmba_surf_extract(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                int n_features, int n_octaves /*1..4*/, float hessian_threshold, int upright /*0 or 1*/,
                int64_t* kp_ptr /*[n_images+1]*/, sfmba_surf_keypoint* kp, float* desc /*[cap][64]*/, int64_t cap, int64_t* total,
                int32_t* dbg_bin /*[cap] or NULL*/, int64_t* dbg_moments /*[cap][2] or NULL*/, int64_t* dbg_sums /*[cap][64] or NULL*/,
                int32_t* dbg_candidates /*[n_images][n_octaves][2] or NULL*/);

/* ---- dense depth maps and a dense cloud: plane-sweep stereo and a consistency filter (SfM::densify) ----------------------------
 * The reference stops at the sparse cloud of the matched key points (its legacy tree densified with optical-flow matches).  Here a
 * list of jobs -- a reference image, 1..4 source images, a depth range -- is swept in one call, and a second call turns the depth
 * maps of a set of images into coloured points.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S; it is stated so that the device is held
 * BIT FOR BIT to a CPU restatement (tests/depth_oracle.py): coordinates are fp64 with EVERY OPERATION ROUNDED ON ITS OWN (no fused
 * multiply-add anywhere; csrc/depth_math.h switches the compiler's contraction off), everything between the coordinate and the score
 * is exact integer arithmetic, the score is a handful of IEEE fp64 operations.  Below, a sum written a + b + c is ((a + b) + c).
 *
 *   images        as sfmba_orb_extract takes them: image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of pixels, height[i] rows of
 *                 width[i] * channels bytes; 3 channels (BGR) are reduced to gray by sfmba_orb_extract's rule
 *                 (1868 b + 9617 g + 4899 r + 8192) >> 14.  Images may differ in size.
 *   cameras       one K [9] row-major of which only fx = K[0], fy = K[4], cx = K[2], cy = K[5] are read; P [n_images][12] row-major
 *                 3 x 4, P = [R | t] with x_cam = R X + t (as sfmba_triangulate_pairs takes them).  Every float is converted to
 *                 double exactly on entry.
 *
 * sfmba_depth_sweep
 *   jobs          job j has the reference image job_ref[j], the sources job_src[job_src_ptr[j] .. job_src_ptr[j+1]-1] (1 to 4,
 *                 distinct, none equal to the reference) and the range 0 < z_near[j] < z_far[j] (finite floats, converted to double).
 *                 Shared: n_planes D in 2..256, radius r in 1..4 (the window holds n = (2r+1)^2 pixels), min_std in 0..127,
 *                 min_score in [-1, 1], min_sources in 1..4.
 *   planes        fronto-parallel to the reference camera, uniform in inverse depth: wn = 1 / z_near, wf = 1 / z_far,
 *                 step = (wn - wf) / (double)(D - 1), w_k = wf + ((double)k step), k = 0 .. D-1 (k = 0 is the far plane).
 *   warp          per (job, source s), on the host: Rrel = R_s R_r^T, trel = t_s - Rrel t_r, M = K Rrel, A = M Kinv, b = K trel with
 *                 K = [fx 0 cx; 0 fy cy; 0 0 1] and Kinv = [1/fx 0 -(cx/fx); 0 1/fy -(cy/fy); 0 0 1].  Every entry of a 3 x 3
 *                 product is (x_i0 y_0j + x_i1 y_1j) + x_i2 y_2j, a matrix-vector product likewise; the zeros and the one of K and
 *                 Kinv take part like any other entry.
 *   sample        for reference pixel (u, v), plane k, source s of size ws x hs: q_i = ((A_i0 u + A_i1 v) + A_i2) + (w_k b_i),
 *                 u' = q_0 / q_2, v' = q_1 / q_2.  VALID iff q_2 > 0, 0 <= u' <= ws-1 and 0 <= v' <= hs-1 (a NaN fails).  Then
 *                 su = (int)floor(16 u' + 0.5), x0 = su >> 4, fx = su & 15, x1 = min(x0 + 1, ws-1), y likewise from v', and
 *                 J = ((16-fx)(16-fy) I00 + fx (16-fy) I10 + (16-fx) fy I01 + fx fy I11 + 8) >> 4 with Iab the source's gray value at
 *                 (x_a, y_b): a 12-bit integer 0..4080.  A sample depends on (u, v, k, s) only, never on the window that reads it.
 *   window        over the (2r+1)^2 pixels around (u, v): SI, SII of the reference's gray values, SJ, SJJ, SIJ of the samples of one
 *                 source.  With r <= 4: SI <= 20655, SII <= 5267025, SJ <= 330480, SIJ <= 84272400, SJJ <= 81 * 4080^2 =
 *                 1348358400 < 2^31.  In int64: varI = n SII - SI^2, varJ = n SJJ - SJ^2, num = n SIJ - SI SJ.
 *   takes part    a reference pixel takes part iff its window lies inside the reference image and varI >= n^2 min_std^2 and varI > 0.
 *   score         source s COUNTS for (pixel, plane) iff all n samples of the window are valid and varJ > 0; its score is then
 *                 (double)num / sqrt((double)varI * (double)varJ): one product, a correctly rounded square root, one division.
 *   plane cost    C_k = (the scores of the counting sources summed in list order, starting from the first) / (double)count; the
 *                 plane is VALID iff count >= min_sources.  k* = the lowest k with the largest C_k among the valid planes.  The
 *                 pixel is ACCEPTED iff a valid plane exists and C_k* >= (double)min_score.
 *   refinement    if 0 < k* < D-1, planes k*-1 and k*+1 are both valid and den = (C- - 2 C0) + C+ < 0 (C-, C0, C+ the costs at
 *                 k*-1, k*, k*+1): delta = (0.5 (C- - C+)) / den; otherwise delta = 0.  w = w_k* + (delta step),
 *                 depth = (float)(1 / w).
 *   outputs       per job, concatenated in job order, each in the reference image's row-major order (the caller sizes them from the
 *                 reference images): depth float [h][w], 0 where the pixel is not accepted; score float [h][w] = (float)C_k*, 0
 *                 where no plane was valid; plane int16 [h][w] = k*, -1 where no plane was valid (may be NULL).  A pixel that does
 *                 not take part has 0, 0, -1.
 *   SFMBA_ERR_INVALID_ARG (nothing written): whatever sfmba_orb_extract refuses about images; fx, fy, cx, cy or a pose entry that is
 *                 not finite, fx or fy <= 0; n_planes, radius, min_std, min_score (NaN included), min_sources outside the ranges
 *                 above; a job whose reference or source index is out of range, that has fewer than 1 or more than 4 sources, that
 *                 lists a source twice or its own reference, or whose range is not 0 < z_near < z_far with both finite; a
 *                 job_src_ptr that does not start at 0.
 *   Host pointers in and out, synchronous.  Deterministic; jobs go to the device in consecutive groups under a fixed scratch bound and
 *   the result does not depend on the grouping: a batch equals the concatenation of single-job calls.
 *
 * sfmba_depth_fuse
 *   inputs        the same images, K and P; depth [n_images]: per image NULL (no map) or a float [h][w] map as the sweep wrote it
 *                 (0 = no depth); per image i the check images chk[chk_ptr[i] .. chk_ptr[i+1]-1] (0 to 4, distinct, none equal to
 *                 i); rel_tol >= 0 (finite), min_consistent in 0..4.
 *   per pixel     (u, v) of image i with z = (double)depth > 0: xn = ((double)u - cx) / fx, yn = ((double)v - cy) / fy,
 *                 d = (z xn - t_0, z yn - t_1, z - t_2), X_j = (R_0j d_0 + R_1j d_1) + R_2j d_2 (R, t of image i).  For check image
 *                 s of size ws x hs: q_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i (R, t of s).  The pixel AGREES with s iff
 *                 q_2 > 0; px = floor(((fx q_0) / q_2 + cx) + 0.5) and py = floor(((fy q_1) / q_2 + cy) + 0.5) satisfy
 *                 0 <= px <= ws-1, 0 <= py <= hs-1 (tested in double; a NaN fails); s has a map; its value zs at (px, py) is > 0; and
 *                 |zs - q_2| <= (double)rel_tol q_2.  The pixel is KEPT iff the number of agreeing check images >= min_consistent.
 *   outputs       the kept pixels in (image, row, column) order: xyz float [cap][3] = (float) of X; bgr uint8 [cap][3] = the pixel's
 *                 own colour (a gray image gives g, g, g); src_image int32 [cap]; src_pixel int32 [cap] = v width + u;
 *                 pt_ptr [n_images + 1].  *total receives the number of points; SFMBA_ERR_CAPACITY (pt_ptr and *total valid,
 *                 nothing else written) if cap < *total.
 *   NO DE-DUPLICATION ACROSS VIEWS: a surface point seen by three views with maps appears three times (sfmba_cloud_merge below
 *                 makes one point per occupied voxel of such a cloud).
 *   SFMBA_ERR_INVALID_ARG (nothing written): what the sweep refuses about images, K and P; rel_tol negative or not finite;
 *                 min_consistent outside 0..4; a check list longer than 4, with an index out of range, a repeated index or the image
 *                 itself; a chk_ptr that does not start at 0; more than 65535 images, or 2^31 or more pixels with a map, in one call.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_depth_sweep(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, int n_jobs, const int32_t* job_ref /*[n_jobs]*/,
                const int64_t* job_src_ptr /*[n_jobs+1]*/, const int32_t* job_src, const float* z_near /*[n_jobs]*/,
                const float* z_far /*[n_jobs]*/, int n_planes /*2..256*/, int radius /*1..4*/, int min_std /*0..127*/,
                float min_score /*[-1, 1]*/, int min_sources /*1..4*/, float* depth, float* score, int16_t* plane /*or NULL*/);
SFMBA_API int sfmba_depth_fuse(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/,
                const int64_t* chk_ptr /*[n_images+1]*/, const int32_t* chk, float rel_tol, int min_consistent /*0..4*/,
                int64_t* pt_ptr /*[n_images+1]*/, float* xyz /*[cap][3]*/, unsigned char* bgr /*[cap][3]*/, int32_t* src_image /*[cap]*/,
                int32_t* src_pixel /*[cap]*/, int64_t cap, int64_t* total);

/* ---- regularised depth maps: semi-global matching over the sweep's cost volume (DenseParams::sgm) -------------------------------
 * sfmba_depth_sweep is winner-take-all per pixel: no pixel hears from its neighbour, and a pixel whose window has no texture gets no
 * depth at all.  These three calls keep the costs of ALL planes, quantised to a byte, and aggregate them along 4 or 8 path directions
 * with a small penalty p1 for a change of one plane and a larger p2 for any other change (semi-global matching, Hirschmueller 2008);
 * a pixel without a cost of its own then takes the plane its neighbours agree on.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S, stated
 * so that the device is held BIT FOR BIT to a CPU restatement (tests/sgm_oracle.py): the cost is the very fp64 value of
 * sfmba_depth_sweep, everything from the quantised cost to the selection is INTEGER arithmetic, and the three fp64 expressions below
 * have every operation rounded on its own (csrc/sgm_math.h switches the compiler's contraction off).
 *
 * sfmba_depth_cost_volume
 *   inputs        images, K, P, jobs, n_planes D, radius, min_std and min_sources exactly as sfmba_depth_sweep takes and refuses them
 *                 (there is no min_score); invalid_cost in 0..254 (checked here; the volume itself does not depend on it).
 *   output        per job, concatenated in job order: cost uint8 [h][w][D], THE PLANE INDEX FASTEST.  Where the pixel takes part and
 *                 plane k is VALID (both as defined under sfmba_depth_sweep) the entry is q = (int)floor((1.0 - C_k) * 127.0 + 0.5),
 *                 0 (C_k = 1) .. 254 (C_k = -1); everywhere else -- an invalid plane, a pixel that does not take part -- it is the
 *                 SENTINEL 255.
 *
 * sfmba_sgm_aggregate
 *   inputs        n_jobs volumes as above: cost[j] uint8 [height[j]][width[j]][D] (host pointers; 1 <= width, height <= 16384;
 *                 one D in 2..256 for all); 0 <= p1 <= p2 <= 1023; n_paths 4 or 8; invalid_cost in 0..254.
 *   cost          c(p, d) = the entry, a sentinel read as invalid_cost: 0..254.
 *   paths         direction r in the order (+1,0), (-1,0), (0,+1), (0,-1) and, with 8 paths, (+1,+1), (-1,-1), (+1,-1), (-1,+1)
 *                 ((dx, dy), y down).  With q = p - r: L_r(p, d) = c(p, d) where q lies outside the image; otherwise
 *                 L_r(p, d) = c(p, d) + min(L_r(q, d), L_r(q, d-1) + p1, L_r(q, d+1) + p1, m + p2) - m with m = min_i L_r(q, i); the
 *                 terms with d-1 < 0 or d+1 > D-1 are left out.  Every term is >= m and m + p2 is always there, so
 *                 0 <= L_r <= 254 + p2 <= 1277.
 *   sums          S(p, d) = sum_r L_r(p, d) <= 8 * 1277 = 10216: a uint16.
 *   selection     k* = the lowest d with the smallest S; best = S(p, k*); second = the smallest S over the d with |d - k*| > 1, or
 *                 0xffff where there is no such d (D = 2, 3 with k* = 1).
 *   outputs       per job (arrays of n_jobs host pointers): plane[j] int16 [h][w] = k*, best[j] and second[j] uint16 [h][w], and
 *                 sums[j] uint16 [h][w][D], the whole S (sums, or any sums[j], may be NULL).
 *   SFMBA_ERR_INVALID_ARG (nothing written): p1, p2, n_paths or invalid_cost outside the ranges above; D outside 2..256; a width or
 *                 height outside 1..16384; n_jobs < 0; a NULL among cost, width, height, plane, best, second or their entries.
 *
 * sfmba_depth_sweep_sgm
 *   inputs        those of sfmba_depth_cost_volume plus p1, p2, n_paths, and uniqueness in 0..100.  The volume and the sums never
 *                 leave the device.
 *   outputs       the three maps of sfmba_depth_sweep in the same layout.  plane = k* for EVERY pixel of the reference image, those
 *                 that do not take part included.  The pixel is ACCEPTED iff second == 0xffff or
 *                 100 (second - best) >= uniqueness second (integers; where all sums are 0 -- a constant cost 0 everywhere -- this holds
 *                 for every uniqueness, and at uniqueness 0 every pixel is accepted).  If 0 < k* < D-1 and den = (S- - 2 S0) + S+ > 0 (integers; S-,
 *                 S0, S+ the sums at k*-1, k*, k*+1) then delta = (0.5 * (double)(S- - S+)) / (double)den, otherwise delta = 0;
 *                 depth = (float)(1 / (w_k* + (delta step))) as in sfmba_depth_sweep, 0 where the pixel is not accepted.
 *                 score = (float)(1.0 - (double)q / 127.0) with q the pixel's OWN volume entry at k*, and 0 where that entry is the
 *                 sentinel: the depth there came from the neighbours alone, and a caller can tell.
 *   equals        sfmba_depth_cost_volume -> sfmba_sgm_aggregate -> the rules above, byte for byte.  Jobs go to the device in
 *                 consecutive groups under sfmba_depth_sweep's scratch bound, which here also counts the volume (1 byte per entry)
 *                 and the sums (2 bytes); a job that exceeds it alone forms a group of its own.  A batch equals the concatenation of
 *                 single-job calls, whatever the grouping.
 *   SFMBA_ERR_INVALID_ARG (nothing written): what sfmba_depth_cost_volume refuses; p1, p2 or n_paths outside the ranges of
 *                 sfmba_sgm_aggregate; uniqueness outside 0..100.
 *   WHAT THIS DOES NOT DO: NO LEFT-RIGHT CHECK -- sfmba_depth_fuse's reprojection filter is the cross-check.  NO ADAPTIVE p2: the
 *                 penalty does not look at the image.  DEPTH IN REGIONS THAT NO SOURCE SEES IS MADE UP FROM THE NEIGHBOURS; only
 *                 `uniqueness` and the fuse stand against it.  The defaults of the host layer (p1 8, p2 64, 8 paths, invalid_cost
 *                 127, uniqueness 5) are FIRST CHOICES THAT NOBODY HAS TUNED.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_depth_cost_volume(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, int n_jobs, const int32_t* job_ref /*[n_jobs]*/,
                const int64_t* job_src_ptr /*[n_jobs+1]*/, const int32_t* job_src, const float* z_near /*[n_jobs]*/,
                const float* z_far /*[n_jobs]*/, int n_planes /*2..256*/, int radius /*1..4*/, int min_std /*0..127*/,
                int min_sources /*1..4*/, int invalid_cost /*0..254*/, unsigned char* cost);
SFMBA_API int sfmba_sgm_aggregate(int device, int n_jobs, const unsigned char* const* cost /*[n_jobs], each [h][w][D]*/,
                const int32_t* width /*[n_jobs]*/, const int32_t* height /*[n_jobs]*/, int n_planes /*2..256*/, int p1, int p2 /*0 <= p1 <= p2 <= 1023*/,
                int n_paths /*4 or 8*/, int invalid_cost /*0..254*/, int16_t* const* plane /*[n_jobs], each [h][w]*/,
                uint16_t* const* best, uint16_t* const* second, uint16_t* const* sums /*or NULL; [n_jobs], each NULL or [h][w][D]*/);
SFMBA_API int sfmba_depth_sweep_sgm(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, int n_jobs, const int32_t* job_ref /*[n_jobs]*/,
                const int64_t* job_src_ptr /*[n_jobs+1]*/, const int32_t* job_src, const float* z_near /*[n_jobs]*/,
                const float* z_far /*[n_jobs]*/, int n_planes /*2..256*/, int radius /*1..4*/, int min_std /*0..127*/,
                int min_sources /*1..4*/, int p1, int p2, int n_paths, int invalid_cost, int uniqueness /*0..100*/, float* depth,
                float* score, int16_t* plane /*or NULL*/);

/* ---- one oriented point per surface element: a normal per depth pixel and the voxel merge (SfM::mergeDenseCloud) ---------------
 * sfmba_depth_fuse leaves a surface point once per view that saw it, and without a normal.  These two calls close the chain from
 * images to a model: a normal per depth pixel, and one point per occupied voxel.  THE CONTRACT IS OUR OWN, stated so that the device
 * is held BIT FOR BIT to a CPU restatement (tests/cloud_oracle.py): per element a handful of fp64 operations, EVERY ONE ROUNDED ON
 * ITS OWN (csrc/cloud_math.h switches the compiler's contraction off), and NOTHING BUT INTEGERS IS SUMMED over a voxel, so the
 * result does not depend on the order of accumulation.  Below, a sum written a + b + c is ((a + b) + c).
 *
 * sfmba_depth_normals
 *   inputs        n_images, width, height, K (only fx, fy, cx, cy are read) and P [n_images][12] as sfmba_depth_fuse takes them;
 *                 depth [n_images]: per image NULL (no map) or a float [h][w] map (0 = no depth); max_rel_step >= 0 (finite).
 *   output        normal [n_images]: per image with a map a float [h][w][3]; a pixel without a normal gets (0, 0, 0).  The entry of
 *                 an image without a map is not read and may be NULL.
 *   per pixel     (u, v) with z0 = (double)depth > 0.  Camera point p(u, v) = (z xn, z yn, z), xn = ((double)u - cx) / fx,
 *                 yn = ((double)v - cy) / fy (the back-projection of the fuse).  A neighbour is USABLE iff it lies inside the image,
 *                 its depth zn > 0 and |zn - z0| <= (double)max_rel_step z0.  du = pE - pW if both (u+1, v) and (u-1, v) are
 *                 usable, pE - p0 if only east is, p0 - pW if only west is, otherwise the pixel has no normal; dv likewise with
 *                 south (v+1) and north (v-1).  c = dv x du, every component (a b) - (c d) with both products rounded.  If
 *                 (c_0 p0_0 + c_1 p0_1) + c_2 p0_2 > 0, c is negated: the normal faces the camera.  len = sqrt((c_0^2 + c_1^2) +
 *                 c_2^2); no normal unless len > 0 and finite.  n_cam = c / len, n_j = (R_0j n_0 + R_1j n_1) + R_2j n_2 with R of the
 *                 image; (float)n_j is stored.
 *   SFMBA_ERR_INVALID_ARG (nothing written): what the fuse refuses about sizes, K and P (a dimension outside 1..16384, a pose entry
 *                 or fx, fy, cx, cy not finite, fx or fy <= 0, more than 65535 images, 2^31 or more pixels with a map);
 *                 max_rel_step negative or not finite; an image with a map and a NULL output.
 *
 * sfmba_cloud_merge
 *   inputs        n points, 0 <= n < 2^31: xyz float [n][3]; bgr uint8 [n][3] or NULL; normal float [n][3] or NULL; voxel > 0
 *                 (a finite float); min_count >= 1.
 *   quantise      per axis a: t = (double)x_a / (double)voxel, q_a = floor(t 1024.0 + 0.5).  A point is SKIPPED iff a coordinate is
 *                 not finite or a q_a lies outside [-2^30, 2^30), tested in double (an infinite or NaN t fails).  Its voxel index
 *                 is i_a = q_a >> 10 (arithmetic: the floor), in [-2^20, 2^20).
 *   key           ((i_x + 2^20) << 42) | ((i_y + 2^20) << 21) | (i_z + 2^20).
 *   normal quanta m_a = floor((double)n_a 16384.0 + 0.5) clamped to [-2^20, 2^20]; a NaN gives 0.
 *   per voxel     over its non-skipped members, c their number: int64 sums Sq_a of q_a, Sb, Sg, Sr of the colours, Sm_a of m_a;
 *                 first = the lowest input index among them.  All sums are integers.  BOUNDS: |q_a| <= 2^30 and c < 2^31 give
 *                 |Sq_a| < 2^61; |m_a| <= 2^20 gives |Sm_a| < 2^51 (exact as a double); a colour sum is < 2^39 and 2 S + c < 2^41.
 *   outputs       the voxels with c >= min_count in ASCENDING KEY order: xyz_out float [cap][3] = (float)((((double)Sq_a /
 *                 (double)c) / 1024.0) (double)voxel); bgr_out = (2 S + c) / (2 c) in integers; normal_out = (float)((double)Sm_a /
 *                 L) with L = sqrt(((double)Sm_0^2 + Sm_1^2) + Sm_2^2), (0, 0, 0) when L == 0; count int32 [cap]; first int32 [cap];
 *                 voxel_of int32 [n] (may be NULL) = the output index of every input point, -1 for a skipped point and for a point
 *                 whose voxel min_count dropped; *total = the number of output voxels; *n_skipped = the number of skipped points.
 *                 SFMBA_ERR_CAPACITY if cap < *total: *total, *n_skipped and voxel_of are valid, nothing else is written.  bgr_out /
 *                 normal_out are not written, and may be NULL, where bgr / normal is NULL.
 *   SFMBA_ERR_INVALID_ARG (nothing written): voxel not finite or <= 0; min_count < 1; n < 0 or n >= 2^31 - 1; cap < 0; a NULL xyz
 *                 with n > 0, total or n_skipped; with cap > 0 a NULL xyz_out, count, first, or the output of a given input.
 *   Both: host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_depth_normals(int device, int n_images, const int32_t* width, const int32_t* height, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/, float max_rel_step,
                float* const* normal /*[n_images], each [h][w][3]; NULL allowed where depth is NULL*/);
SFMBA_API int sfmba_cloud_merge(int device, int64_t n, const float* xyz /*[n][3]*/, const unsigned char* bgr /*[n][3] or NULL*/,
                const float* normal /*[n][3] or NULL*/, float voxel, int min_count, float* xyz_out /*[cap][3]*/,
                unsigned char* bgr_out /*[cap][3]*/, float* normal_out /*[cap][3]*/, int32_t* count /*[cap]*/, int32_t* first /*[cap]*/,
                int32_t* voxel_of /*[n] or NULL*/, int64_t cap, int64_t* total, int64_t* n_skipped);

/* ---- a surface from the depth maps: TSDF fusion and marching tetrahedra (SfM::meshDenseCloud) ------------------------------------
 * The clouds above are a weak basis for a surface: the fuse leaves a surface element once per view, and the depth error keeps the
 * duplicates apart.  These three calls average the depth maps along the viewing rays in a truncated signed distance grid and take
 * the zero set of the grid out as a triangle mesh.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S, stated so that the device is held
 * BIT FOR BIT to a CPU restatement (tests/mesh_oracle.py): fp64 with EVERY OPERATION ROUNDED ON ITS OWN (csrc/mesh_math.h switches
 * the compiler's contraction off), and NOTHING BUT INTEGERS IS SUMMED per voxel, so the result does not depend on the order of the
 * images or of accumulation.  Below, a sum written a + b + c is ((a + b) + c).
 *
 * the grid        origin float [3] (finite), voxel > 0 (a finite float), nx, ny, nz each in 1..1024 with nx ny nz <= 2^26.  Grid
 *                 vertex (i, j, k) lies at G_a = (double)origin_a + ((double)i_a (double)voxel); lin = (k ny + j) nx + i.
 *
 * sfmba_tsdf_integrate
 *   inputs        images, K, P and depth [n_images] (each NULL or a float [h][w] map, 0 = no depth) as sfmba_depth_fuse takes them,
 *                 except that pixels may be NULL (no colour; img_ptr and channels are then not read); trunc > 0 (a finite float),
 *                 T = (double)trunc.
 *   per vertex X and per image s with a map: q_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i, needing q_2 > 0; the pixel
 *                 px = floor(((fx q_0) / q_2 + cx) + 0.5), py likewise, both inside the image (tested in double; a NaN fails): the
 *                 fuse's rule, one copy of the code; zs = (double)map[py][px] > 0; sdf = zs - q_2.  The image CONTRIBUTES iff
 *                 sdf >= -T, with e = (int)floor((min(sdf, T) / T) 1024.0 + 0.5) in [-1024, 1024]: S += e, W += 1.  If also sdf <= T
 *                 and pixels is given: Sb, Sg, Sr += the pixel's colour (a gray image gives g, g, g), Wc += 1.
 *                 BOUNDS: at most 65535 images, so |S| < 2^26 and a colour sum < 2^24; everything is int32.
 *   outputs       sum int32 [nz][ny][nx], weight int32 [nz][ny][nx]; csum int32 [nz][ny][nx][3] and cweight int32 [nz][ny][nx]:
 *                 both given or both NULL, and both untouched when pixels is NULL.
 *
 * sfmba_tsdf_extract
 *   inputs        such a grid from the host (csum and cweight both given or both NULL) and min_weight in 1..65535.
 *   cells         a vertex is DEFINED iff W >= min_weight, its value is f = (double)S / (double)W, it is INSIDE iff S < 0.  Cell
 *                 (i, j, k) exists for i < nx-1, j < ny-1, k < nz-1 and is ACTIVE iff all eight corners are defined.
 *   tetrahedra    an active cell is split into the six tetrahedra of Kuhn's triangulation: tetrahedron p in 0..5 is the p-th
 *                 permutation (a, b, c) of the axes (0, 1, 2) in lexicographic order, with local vertices v0 = corner,
 *                 v1 = v0 + e_a, v2 = v1 + e_b, v3 = corner + (1, 1, 1).  Every edge runs from a grid vertex A to A + d, d in
 *                 {0, 1}^3 \ {0}; its KEY is lin(A) * 8 + (d_x + 2 d_y + 4 d_z - 1) < 2^29.  Neighbouring cells split their common
 *                 face alike.
 *   triangles     I, O = the inside and the outside local indices, ascending; nothing if either is empty.  |I| = 1: one triangle
 *                 on the edges (I0, O0), (I0, O1), (I0, O2).  |I| = 3: (I0, O0), (I1, O0), (I2, O0).  |I| = 2: the cycle
 *                 c0 = (I0, O0), c1 = (I0, O1), c2 = (I1, O1), c3 = (I1, O0) gives (c0, c1, c2) then (c0, c2, c3).  ORIENTATION, in
 *                 integers on the unit cell: with the doubled edge midpoints m = v_x + v_y of a triangle (A, B, C),
 *                 n = (B - A) x (C - A) and d = |I| sum_{o in O} v_o - |O| sum_{i in I} v_i; if n . d < 0 the last two vertices are
 *                 swapped (the product is never 0); then the triangle is rotated so that its lowest key comes first.  Normals face
 *                 the outside, towards the cameras.  ORDER: cells in ascending lin of their corner, tetrahedra 0..5, then as above.
 *   vertices      the keys that some triangle uses, in ASCENDING KEY ORDER.  With A the lower end and B = A + d:
 *                 t = fA / (fA - fB), pos_a = (double)origin_a + (((double)i_a + (t (double)d_a)) (double)voxel), stored as (float);
 *                 colour per channel (2 (S_A + S_B) + w) / (2 w) in integers with w = Wc_A + Wc_B, (0, 0, 0) when w == 0.
 *                 Degenerate triangles are kept: S == 0 at a corner gives t == 0, so several keys land on one position.
 *   outputs       xyz float [vcap][3]; bgr uint8 [vcap][3] (not written, and may be NULL, where csum is NULL); vkey int32 [vcap]
 *                 (may be NULL); tri int32 [tcap][3], indices into the vertex list; *n_vertices, *n_triangles.
 *                 SFMBA_ERR_CAPACITY if vcap < *n_vertices or tcap < *n_triangles: both totals are valid, nothing else is written.
 *
 * sfmba_tsdf_mesh
 *   the inputs of integrate and min_weight, the outputs of extract, the grid never leaving the device; colour iff pixels is given.
 *   EQUALS sfmba_tsdf_integrate FOLLOWED BY sfmba_tsdf_extract BYTE FOR BYTE.
 *
 *   SFMBA_ERR_INVALID_ARG (nothing written): whatever the fuse refuses about images, sizes, K and P (more than 65535 images and 2^31
 *                 or more pixels with a map included); an origin that is not finite; voxel or trunc not finite or <= 0; a dimension
 *                 outside 1..1024 or more than 2^26 voxels; min_weight outside 1..65535; in a grid handed to extract a negative
 *                 weight or cweight, |S| > 1024 W, or a colour sum outside 0..255 Wc (found on the device, before anything is
 *                 written); a negative capacity; a NULL origin, sum, weight, n_vertices, n_triangles, depth with n_images > 0, xyz
 *                 (or bgr, where colours are made) with vcap > 0, tri with tcap > 0; csum without cweight or the reverse.
 *   All three: host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_tsdf_integrate(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels /*or NULL*/, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/,
                const float* origin /*[3]*/, float voxel, int nx, int ny, int nz, float trunc, int32_t* sum /*[nz][ny][nx]*/,
                int32_t* weight /*[nz][ny][nx]*/, int32_t* csum /*[nz][ny][nx][3] or NULL*/, int32_t* cweight /*[nz][ny][nx] or NULL*/);
SFMBA_API int sfmba_tsdf_extract(int device, const float* origin /*[3]*/, float voxel, int nx, int ny, int nz,
                const int32_t* sum /*[nz][ny][nx]*/, const int32_t* weight /*[nz][ny][nx]*/, const int32_t* csum /*[nz][ny][nx][3] or NULL*/,
                const int32_t* cweight /*[nz][ny][nx] or NULL*/, int min_weight /*1..65535*/, float* xyz /*[vcap][3]*/,
                unsigned char* bgr /*[vcap][3]*/, int32_t* vkey /*[vcap] or NULL*/, int64_t vcap, int32_t* tri /*[tcap][3]*/, int64_t tcap,
                int64_t* n_vertices, int64_t* n_triangles);
SFMBA_API int sfmba_tsdf_mesh(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels /*or NULL*/, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/,
                const float* origin /*[3]*/, float voxel, int nx, int ny, int nz, float trunc, int min_weight /*1..65535*/,
                float* xyz /*[vcap][3]*/, unsigned char* bgr /*[vcap][3]*/, int32_t* vkey /*[vcap] or NULL*/, int64_t vcap,
                int32_t* tri /*[tcap][3]*/, int64_t tcap, int64_t* n_vertices, int64_t* n_triangles);

/* ---- filling the holes of the surface: volumetric diffusion of the TSDF grid (MeshParams::fillIterations) -------------------------
 * A cell of the extraction is active only if all eight corners are defined, so the zero set stops one cell short of every undefined
 * vertex: behind every seen surface, at grazing angles and wherever a depth map has a hole, and the mesh of the calls above is OPEN.
 * These two calls diffuse the signed distance into the undefined vertices (Davis et al., "Filling holes in complex surfaces using
 * volumetric diffusion") and leave sfmba_tsdf_extract exactly as it is.  The integration marks seen free space (sdf > T contributes
 * e = 1024), so the unknown region is bounded by "outside" wherever a camera looked.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S,
 * stated so that the device is held BIT FOR BIT to a CPU restatement (tests/tsdf_fill_oracle.py): NOTHING BUT INTEGERS
 * (csrc/tsdf_fill_math.h).  Below, floor_div rounds towards minus infinity.  UNSEEN GEOMETRY CANNOT BE INVENTED: AT AN OPEN BORDER
 * THE FILL CONTINUES THE SURFACE AS A SKIRT UP TO `iterations` VOXELS WIDE, so the feature is OFF BY DEFAULT, has two knobs (NOT
 * TUNED) and says per vertex what it made up.
 *
 * sfmba_tsdf_fill
 *   inputs        a grid as sfmba_tsdf_extract takes it (nx, ny, nz, sum, weight, and csum / cweight both or neither; the origin and
 *                 the voxel are not needed), min_weight in 1..65535, iterations in 0..254, min_neighbours in 1..6.
 *   definitions   a vertex is OBSERVED iff W >= min_weight.  Its value is V = floor_div(128 S + W, 2 W): 64 S / W rounded half up, in
 *                 -65536..65536.  Its colour is c = (2 Sc + Wc) / (2 Wc) per channel, with hasC = (Wc > 0).  Every other vertex
 *                 starts UNKNOWN, one with 0 < W < min_weight included.  KNOWN means observed, or filled in an earlier pass.
 *   a pass        every vertex reads the state from BEFORE the pass (Jacobi; no atomic).  For a vertex that is not observed: n6 = the
 *                 number of its KNOWN face neighbours, at most 6 (neighbours outside the grid do not exist).  An unknown vertex
 *                 becomes known in this pass iff n6 >= min_neighbours.  A vertex that is already known and filled is updated in
 *                 every pass (its n6 can no longer drop to 0).  The new value is V' = floor_div(2 sum V + n, 2 n), the sum over its
 *                 known face neighbours and over itself if it was known, n the number of terms, at most 7.  Colour: among those
 *                 same terms take the m with hasC; if m > 0 then c' = (2 sum c + m) / (2 m) per channel and hasC' = 1, otherwise
 *                 hasC' = 0.  Observed vertices never change.  BOUNDS: |sum V| <= 7 * 65536; everything fits int32.
 *   outputs       sum_out, weight_out, and csum_out / cweight_out where the input has them.  An observed or still-unknown vertex is
 *                 copied BIT FOR BIT (with iterations == 0 the output is the input).  A filled vertex gets W = FW = 64 ceil(min_weight
 *                 / 64), in 64..65536, so it is defined for the extraction at the same min_weight; S = V (FW / 64), so S / W = V / 64
 *                 exactly and |S| <= 1024 W; csum = c and cweight = 1 if hasC, else zeros.  state uint8 [nz][ny][nx] (may be NULL):
 *                 0 for observed, p in 1..254 for the pass in which the vertex became known, 255 for still unknown.  *n_filled.
 *   DERIVABLE     a vertex with state == p lies within L1 distance p of an observed vertex.  So no mesh vertex made by the fill lies
 *                 farther than iterations + 1 voxels (L1) from an observed grid vertex: the width of the skirt at an open border.
 *
 * sfmba_tsdf_mesh_fill
 *   the arguments of sfmba_tsdf_mesh, plus fill_iterations and min_neighbours, plus vfilled uint8 [vcap] (may be NULL): 1 iff either
 *   end of the mesh vertex's edge is a filled grid vertex.  Integrates, fills and extracts, the grid never leaving the device.
 *   EQUALS sfmba_tsdf_integrate, sfmba_tsdf_fill, sfmba_tsdf_extract BYTE FOR BYTE.  With fill_iterations == 0 it equals
 *   sfmba_tsdf_mesh byte for byte and vfilled is all 0.  The capacity protocol is the extraction's (vfilled is not written either).
 *
 *   SFMBA_ERR_INVALID_ARG (nothing written): whatever sfmba_tsdf_extract (for the combined call: sfmba_tsdf_mesh) refuses about the
 *                 dimensions, min_weight and the grid's contents (found on the device, before anything is written); iterations
 *                 outside 0..254; min_neighbours outside 1..6; a NULL sum, weight, sum_out, weight_out or n_filled; csum without
 *                 cweight or the reverse; colour outputs missing where colour inputs are given.
 *   IN-PLACE IS NOT SUPPORTED.  Both: host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding
 *   symbols is backward compatible.
 */
SFMBA_API int sfmba_tsdf_fill(int device, int nx, int ny, int nz, const int32_t* sum /*[nz][ny][nx]*/, const int32_t* weight /*[nz][ny][nx]*/,
                const int32_t* csum /*[nz][ny][nx][3] or NULL*/, const int32_t* cweight /*[nz][ny][nx] or NULL*/, int min_weight /*1..65535*/,
                int iterations /*0..254*/, int min_neighbours /*1..6*/, int32_t* sum_out, int32_t* weight_out, int32_t* csum_out /*or NULL*/,
                int32_t* cweight_out /*or NULL*/, unsigned char* state /*[nz][ny][nx] or NULL*/, int64_t* n_filled);
SFMBA_API int sfmba_tsdf_mesh_fill(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels /*or NULL*/, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                const float* K /*[9]*/, const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/,
                const float* origin /*[3]*/, float voxel, int nx, int ny, int nz, float trunc, int min_weight /*1..65535*/,
                int fill_iterations /*0..254*/, int min_neighbours /*1..6*/, float* xyz /*[vcap][3]*/, unsigned char* bgr /*[vcap][3]*/,
                int32_t* vkey /*[vcap] or NULL*/, unsigned char* vfilled /*[vcap] or NULL*/, int64_t vcap, int32_t* tri /*[tcap][3]*/,
                int64_t tcap, int64_t* n_vertices, int64_t* n_triangles);

/* ---- cleaning a mesh: components, small-island removal, Taubin smoothing, vertex normals (SfM::cleanMesh) ------------------------
 * The mesh of the calls above is a set of open sheets with islands: a depth outlier that survives the fuse is a floating shell of a
 * few dozen triangles, and the surface carries the plane-step noise of the sweep.  These four calls label the connected components,
 * drop the small ones, smooth without shrinking (Taubin's lambda | mu) and give every vertex a normal.  THE CONTRACT IS OUR OWN AND
 * EQUALS NOBODY'S, stated so that the device is held BIT FOR BIT to a CPU restatement (tests/mesh_clean_oracle.py): positions are
 * quantised to integers once, a pass is integer arithmetic with one floor division per axis, the few fp64 operations are EVERY ONE
 * ROUNDED ON ITS OWN (csrc/mesh_clean_math.h switches the compiler's contraction off), and NOTHING BUT INTEGERS IS SUMMED ACROSS
 * TRIANGLES, so the result depends neither on the order in which atomics arrive nor on how the work is cut.  Below, a sum written
 * a + b + c is ((a + b) + c).
 *
 * the mesh        n_vertices >= 0 and n_triangles >= 0, both < 2^31; xyz float [n_vertices][3]; bgr uint8 [n_vertices][3] or NULL;
 *                 tri int32 [n_triangles][3], indices into 0 .. n_vertices-1.
 *
 * sfmba_mesh_components
 *   rule          two vertices are connected when some triangle names both; a triangle with a repeated index still connects the
 *                 indices it names.  A triangle BELONGS to the component of its first index.
 *   outputs       label int32 [n_vertices]: the lowest vertex index of the vertex's component (a vertex that no triangle names is
 *                 its own label); comp_triangles int32 [n_vertices] (may be NULL): the number of triangles of the vertex's
 *                 component, 0 for an unused vertex; *n_components: the labels that own at least one triangle; *largest: the label
 *                 with the most triangles, ties to the LOWER label, -1 if there is no triangle.
 *
 * sfmba_mesh_filter
 *   inputs        the mesh, min_triangles >= 1, keep_largest in {0, 1}.
 *   rule          a component is KEPT iff its triangle count >= min_triangles and, with keep_largest, it also is `largest` (so
 *                 nothing is kept when min_triangles exceeds the largest count).  A triangle is kept iff its component is; a vertex
 *                 is kept iff a kept triangle names it.  Kept vertices and kept triangles KEEP THEIR RELATIVE ORDER; triangle indices
 *                 are rewritten to the new numbering.  min_triangles = 1, keep_largest = 0 removes exactly the unused vertices.
 *   outputs       xyz_out float [vcap][3]; bgr_out uint8 [vcap][3] (not written, and may be NULL, where bgr is NULL); tri_out int32
 *                 [tcap][3]; vertex_of int32 [n_vertices] (may be NULL): the new index of a vertex or -1; *n_vertices_out,
 *                 *n_triangles_out.  SFMBA_ERR_CAPACITY if vcap < *n_vertices_out or tcap < *n_triangles_out: both totals are valid,
 *                 nothing else is written.
 *
 * sfmba_mesh_smooth
 *   inputs        xyz, tri; origin float [3] (finite) and quantum > 0 (a finite float); iterations in 0..100; lambda, mu (floats).
 *   quantisation  L = (int)floor((double)lambda 65536 + 0.5) in 1..65536 and M likewise from mu in -131072..-1.
 *                 P_a = (int64)floor(((double)x_a - (double)origin_a) / (double)quantum + 0.5); every coordinate must be finite with
 *                 |P_a| < 2^25.
 *   a pass with factor F   for every triangle (a, b, c) whose three indices are DISTINCT: S_a += P_b + P_c, D_a += 2, and the same
 *                 for b and c (integers only; an interior edge of a manifold mesh counts twice and a boundary edge once: on a closed
 *                 manifold this is the uniform umbrella).  A vertex with D = 0 or D > 2^17 does not move.  Otherwise per axis
 *                 n = F (S - D P), den = D 65536, P' = P + floor_div(2 n + den, 2 den): round half up, floor semantics for
 *                 negatives; with |P| < 2^25 and D <= 2^17, |2 n + den| < 2^62.  If |P'_a| >= 2^25 on some axis the vertex does not
 *                 move in this pass either (only a mu near -2 on a spike at the rim of the range gets there; every pass then starts
 *                 from |P| < 2^25 and the bounds above hold throughout).  Every vertex reads the positions from before the pass.
 *   an iteration  a pass with L, then a pass with M.
 *   positions     xyz_out_a = (float)((double)origin_a + ((double)P_a (double)quantum)); with iterations == 0, xyz_out is xyz BIT FOR
 *                 BIT (the range check still applies).
 *   normals       normal float [n_vertices][3], may be NULL; from the final integer positions (with iterations == 0 the quantised
 *                 input).  Per triangle with distinct indices N = (P_b - P_a) x (P_c - P_a) in int64 (differences < 2^26, products
 *                 < 2^52, components < 2^53, so (double)N is exact); len = sqrt((Nx Nx + Ny Ny) + Nz Nz); a triangle with len == 0
 *                 adds nothing; otherwise u_a = (int64)floor((N_a / len) 1048576.0 + 0.5) is added to each of its three vertices.
 *                 The vertex normal is (float)(U_a / sqrt((Ux Ux + Uy Uy) + Uz Uz)) with U as doubles, (0, 0, 0) for a zero sum.
 *                 EVERY TRIANGLE HAS EQUAL WEIGHT: THE NORMALS ARE NOT AREA WEIGHTED.
 *
 * sfmba_mesh_clean
 *   the inputs of filter and of smooth, the outputs of filter and normal float [vcap][3] (may be NULL), the mesh never leaving the
 *   device, colours carried through.  EQUALS sfmba_mesh_filter FOLLOWED BY sfmba_mesh_smooth BYTE FOR BYTE; the range check sees the
 *   kept vertices only, and comes after the capacity protocol.
 *
 *   SFMBA_ERR_INVALID_ARG (nothing written): a negative or >= 2^31 count; a triangle index outside the vertex list (found on the
 *                 device, before anything is written); min_triangles < 1; keep_largest outside {0, 1}; iterations outside 0..100;
 *                 L or M outside its range (a NaN included); an origin that is not finite; quantum not finite or <= 0; a coordinate
 *                 that is not finite or has |P_a| >= 2^25 (found on the device, before anything is written); a negative capacity;
 *                 a NULL tri with n_triangles > 0, xyz, label or the smooth's xyz_out with n_vertices > 0, origin, n_components,
 *                 largest, n_vertices_out, n_triangles_out, xyz_out (or bgr_out, where bgr is given) with vcap > 0, tri_out with
 *                 tcap > 0.
 *   All four: host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_mesh_components(int device, int64_t n_vertices, int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/,
                int32_t* label /*[n_vertices]*/, int32_t* comp_triangles /*[n_vertices] or NULL*/, int64_t* n_components, int64_t* largest);
SFMBA_API int sfmba_mesh_filter(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int min_triangles /*>= 1*/, int keep_largest /*0, 1*/,
                float* xyz_out /*[vcap][3]*/, unsigned char* bgr_out /*[vcap][3]*/, int64_t vcap, int32_t* tri_out /*[tcap][3]*/, int64_t tcap,
                int32_t* vertex_of /*[n_vertices] or NULL*/, int64_t* n_vertices_out, int64_t* n_triangles_out);
SFMBA_API int sfmba_mesh_smooth(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, int64_t n_triangles,
                const int32_t* tri /*[n_triangles][3]*/, const float* origin /*[3]*/, float quantum, int iterations /*0..100*/, float lambda,
                float mu, float* xyz_out /*[n_vertices][3]*/, float* normal /*[n_vertices][3] or NULL*/);
SFMBA_API int sfmba_mesh_clean(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int min_triangles /*>= 1*/, int keep_largest /*0, 1*/,
                const float* origin /*[3]*/, float quantum, int iterations /*0..100*/, float lambda, float mu, float* xyz_out /*[vcap][3]*/,
                unsigned char* bgr_out /*[vcap][3]*/, float* normal /*[vcap][3] or NULL*/, int64_t vcap, int32_t* tri_out /*[tcap][3]*/,
                int64_t tcap, int32_t* vertex_of /*[n_vertices] or NULL*/, int64_t* n_vertices_out, int64_t* n_triangles_out);

/* ---- decimating a mesh: vertex clustering with quadric placement (SfM::decimateMesh) ----------------------------------------------
 * Marching tetrahedra emits triangles far smaller than a pixel's footprint, and everything after the mesh (the view choice, the
 * atlas, the label smoothing, the colour levelling) pays per triangle.  This call hands those stages fewer, larger triangles: every
 * vertex falls into a cubic cell of `cell` quanta, a cell's vertices become ONE representative, and the triangles that survive are
 * those whose three vertices lie in three different cells (out-of-core vertex clustering, Lindstrom 2000).  The representative is
 * either the rounded mean of the members or the minimiser of the cell's quadric (the summed squared distances to the planes of the
 * incident triangles), which keeps the edges and corners that a mean rounds off.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S, stated
 * so that the device is held BIT FOR BIT to a CPU restatement (tests/decimate_oracle.py): NOTHING BUT INTEGERS IS SUMMED ACROSS
 * VERTICES OR TRIANGLES, the few fp64 operations are EVERY ONE ROUNDED ON ITS OWN (csrc/decimate_math.h switches the compiler's
 * contraction off), and a sum written a + b + c is ((a + b) + c).
 *
 *   inputs        the mesh of the cleaning calls; origin float [3] (finite) and quantum > 0 (a finite float); cell in 32..2^20, in
 *                 quanta; placement 0 (mean) or 1 (quadric); reg in 1..2^20, read only with placement 1.
 *   quantisation  P_a exactly as sfmba_mesh_smooth computes it, with the same refusal of a coordinate that is not finite or has
 *                 |P_a| >= 2^25.
 *   cell and key  c_a = floor_div(P_a, cell), r_a = P_a - c_a cell in 0..cell-1; with cell >= 32, c_a lies in [-2^20, 2^20).
 *                 key = ((c_z + 2^20) << 42) | ((c_y + 2^20) << 21) | (c_x + 2^20).  Every vertex is a member of its cell's cluster,
 *                 whether or not a triangle names it.
 *   mean          for a cluster of n members Sp_a = the sum of r_a over the members (< 2^51); R_a = floor_div(2 Sp_a + n, 2 n).  A
 *                 colour channel is the same rounded mean over the members' bytes.
 *   quadric       (placement 1) a triangle contributes when its three indices are DISTINCT and its normal is non-zero:
 *                 N = (P_b - P_a) x (P_c - P_a) in int64 and len = sqrt((Nx Nx + Ny Ny) + Nz Nz) as in the smooth's normals;
 *                 u_a = (int64)floor((N_a / len) 1024.0 + 0.5), |u_a| <= 1024.  EVERY TRIANGLE HAS EQUAL WEIGHT: THE QUADRICS ARE
 *                 NOT AREA WEIGHTED.  For each of its three vertices v, into the cluster of v, with v's own r:
 *                 e = (u_x r_x + u_y r_y) + u_z r_z (|e| < 2^32); A_ij += u_i u_j (six entries); b_i += u_i e; n_inc += 1.
 *                 A cluster takes the mean's R when n_inc == 0 or n_inc > 2^16 (counted in stats).  Up to that cap |A_ij| <= 2^36
 *                 and |b_i| < 2^58.
 *   the solve     in doubles: rho = (double)reg (double)n_inc; m_a = (double)Sp_a / (double)n; s = (double)A + rho I;
 *                 g_a = (double)b_a + rho m_a.  Cofactors c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11,
 *                 c11 = s00 s22 - s02 s02, c12 = s01 s02 - s00 s12, c22 = s00 s11 - s01 s01; det = (s00 c00 + s01 c01) + s02 c02;
 *                 x_0 = ((c00 g0 + c01 g1) + c02 g2) / det, x_1 and x_2 likewise from the symmetric adjugate.  If !(det > 0) or an
 *                 x_a is not finite the cluster takes the mean's R (counted in stats); otherwise
 *                 R_a = clamp((int64)floor(x_a + 0.5), 0, cell - 1): A REPRESENTATIVE NEVER LEAVES ITS CELL.  The regulariser pulls
 *                 towards the members' mean with weight reg / 2^20 relative to a unit normal.
 *   position      xyz_out_a = (float)((double)origin_a + ((double)(c_a cell + R_a) (double)quantum)).
 *   triangles     a triangle is COLLAPSED when two of its vertices share a cluster (a repeated index is one such case).  Among the
 *                 others with the same UNORDERED triple of clusters the lowest input index survives, whatever the orientation.
 *                 Survivors keep their relative order and their index order (so their orientation).  A cluster is emitted iff a
 *                 surviving triangle names it; clusters are emitted in ASCENDING KEY ORDER.
 *   outputs       xyz_out float [vcap][3]; bgr_out uint8 [vcap][3] (not written, and may be NULL, where bgr is NULL); members int32
 *                 [vcap] (may be NULL): a cluster's member count; tri_out int32 [tcap][3]; triangle_of int32 [tcap] (may be NULL):
 *                 the input index of an output triangle; vertex_of int32 [n_vertices] (may be NULL): the output index of a vertex's
 *                 cluster or -1; *n_vertices_out, *n_triangles_out; stats int64 [4] (may be NULL) = { clusters before the emit rule,
 *                 collapsed triangles, duplicates dropped, clusters with placement 1 that took the mean }.
 *                 SFMBA_ERR_CAPACITY if vcap < *n_vertices_out or tcap < *n_triangles_out: both totals are valid, nothing else is
 *                 written.
 *   SFMBA_ERR_INVALID_ARG (nothing written): what sfmba_mesh_filter and sfmba_mesh_smooth refuse about the mesh, origin, quantum,
 *                 the capacities and the pointers (the index and coordinate checks run on the device, before anything is written);
 *                 cell outside 32..2^20; placement outside {0, 1}; reg outside 1..2^20 when placement is 1.
 *   NOT DONE: no edge-collapse simplification, no topology guarantee (sheets closer than a cell fuse, a few non-manifold edges
 *   appear on a clean solid and thousands on the noisy open sheets of a reconstruction: profiles/mesh_decimate.txt), no area
 *   weighting, no boundary-preserving quadrics.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding a symbol is backward compatible.
 */
SFMBA_API int sfmba_mesh_decimate(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, const float* origin /*[3]*/, float quantum,
                int cell /*32..2^20, in quanta*/, int placement /*0 mean, 1 quadric*/, int reg /*1..2^20; read only with placement 1*/,
                float* xyz_out /*[vcap][3]*/, unsigned char* bgr_out /*[vcap][3]*/, int32_t* members /*[vcap] or NULL*/, int64_t vcap,
                int32_t* tri_out /*[tcap][3]*/, int32_t* triangle_of /*[tcap] or NULL: input index of an output triangle*/, int64_t tcap,
                int32_t* vertex_of /*[n_vertices] or NULL*/, int64_t* n_vertices_out, int64_t* n_triangles_out, int64_t* stats /*[4] or NULL*/);

/* ---- texturing a mesh: a view per triangle and a texture atlas of fixed-size patches (SfM::textureMesh) ---------------------------
 * A vertex of the meshes above has one colour: the mean over all views of the pixels that fell into the two grid vertices of its
 * edge, blurred by the voxel and by views that disagree by the depth error, and no finer than the grid.  This call puts the
 * photographs themselves on the surface: every triangle chooses ONE view, the one that sees it largest among those that see it at
 * all, and gets a right-angled patch of S x S texels in an atlas, filled from that view by a perspective-correct bilinear fetch.  The
 * triangles of a grid mesh are all about the same size, so a FIXED-SIZE PATCH PER TRIANGLE is the atlas and nothing is packed.  THE
 * CONTRACT IS OUR OWN AND EQUALS NOBODY'S, stated so that the device is held BIT FOR BIT to a CPU restatement
 * (tests/texture_oracle.py): fp64 per element, EVERY OPERATION ROUNDED ON ITS OWN (csrc/texture_math.h switches the compiler's
 * contraction off), and everything from the fixed-point image coordinate to the texel is integer arithmetic.  Nothing is summed
 * across triangles or texels and there is NO ATOMIC ANYWHERE.  Below, a sum written a + b + c is ((a + b) + c).
 *
 * sfmba_mesh_texture
 *   the mesh      as the mesh-cleaning calls take it: xyz, bgr (or NULL), tri.
 *   the views     images, K, P and the depth maps exactly as sfmba_depth_fuse / sfmba_tsdf_integrate take them (the pixels are
 *                 required; depth[i] may be NULL: such a view has no visibility test).  n_images = 0 is legal.
 *   parameters    occl_tol >= 0 (a finite float, world units); min_area >= 0 in (1/16 px)^2, DOUBLED; the patch S in 3..64; the
 *                 blocks per atlas row B >= 1.
 *   layout        triangle t lives in block b = t >> 1, half t & 1.  n_blocks = ceil(n_triangles / 2); W = B (S + 1),
 *                 H = ceil(n_blocks / B) S; both must lie in 1..16384.  With n_triangles = 0 the atlas is ONE EMPTY BLOCK, S + 1 by
 *                 S, whatever B, and all zero.  Block b has its origin at ((b mod B)(S + 1), (b / B) S).  Half 0 owns the local
 *                 texels (i, j), 0 <= i, j < S, i + j <= S - 1.  Half 1 is the block turned by 180 degrees: its local texel (x, y) is
 *                 its own frame's (i, j) = (S - x, S - 1 - y).  Both halves have S (S + 1) / 2 texels and every texel of a block
 *                 belongs to exactly one half.  The corners A, B, C of a triangle sit on the texel CENTRES (0, 0), (S - 2, 0),
 *                 (0, S - 2) of the half's own frame; the owned texels beyond the hypotenuse and the legs are extrapolated, so a
 *                 bilinear fetch inside the uv triangle never reads a texel of the other half (the gutter).  uv float
 *                 [n_triangles][3][2] holds the three corners in atlas pixel units, exact values integer + 0.5, origin top-left; the
 *                 caller normalises.  Texels that no triangle owns (the second half of the last block of an odd n_triangles, the
 *                 blocks past n_blocks in the last row) are 0.
 *   view choice   per triangle, views in ascending index.  A vertex X = (double) of its floats PASSES in a view iff q = R X + t (the
 *                 fuse's rule, q_i = ((R_i0 X_0 + R_i1 X_1) + R_i2 X_2) + t_i) has q_2 > 0; u = (fx q_0) / q_2 + cx and
 *                 v = (fy q_1) / q_2 + cy lie in [0, w - 1] and [0, h - 1] (a NaN fails); and, where the view has a map, at the pixel
 *                 (floor(u + 0.5), floor(v + 0.5)) zs = (double)map[py][px] > 0 and (q_2 - zs) <= (double)occl_tol.  The view is a
 *                 CANDIDATE iff all three vertices pass.  With su = floor(16 u + 0.5), sv likewise (the sweep's fixed point), the
 *                 doubled signed image area in int64 is a2 = (suB - suA)(svC - svA) - (svB - svA)(suC - suA); for fx, fy > 0 a
 *                 triangle whose normal (B - A) x (C - A) points towards the camera has a2 < 0 (image y runs down).  score = -a2.
 *                 The view is ELIGIBLE iff it is a candidate, score > 0 and score >= min_area.  view[t] is the eligible view of
 *                 largest score, the LOWEST INDEX ON A TIE, or -1; score[t] (may be NULL) is that score, or 0.  A triangle with a
 *                 non-finite coordinate or a repeated index gets -1.  *n_textured is the number of triangles with view >= 0.
 *   texels        per owned texel (i, j) of the half's frame: wB = i, wC = j, wA = S - 2 - i - j (the least is -1);
 *                 X_a = (((double)wA A_a + (double)wB B_a) + (double)wC C_a) / (double)(S - 2): interpolating in 3-D makes the
 *                 mapping perspective-correct.  With view >= 0: q, u, v as above; if q_2 > 0 and neither u nor v is a NaN, both are
 *                 clamped into the image, su and sv are taken as above, and channel c of the texel is (s12 + 8) >> 4 with s12 the
 *                 sweep's bilinear sample (0..4080) of that channel at (su, sv) / 16; a gray image gives g, g, g.  Otherwise, and
 *                 for a triangle with view = -1, the texel takes the FALLBACK: per channel
 *                 floor((2 (wA cA + wB cB + wC cC) + (S - 2)) / (2 (S - 2))) in integers, clamped to 0..255, with cA, cB, cC the
 *                 corners' bgr -- a FLOOR division, not a truncation -- and (0, 0, 0) where bgr is NULL.
 *   outputs       atlas uint8 [H][W][3], BGR; uv; view int32 [n_triangles]; score int64 [n_triangles] or NULL; *n_textured.
 *   NO COLOUR ADJUSTMENT ACROSS VIEWS unless asked for (off by default), see "levelling the colours across seams" below: SEAMS WHERE
 *   EXPOSURES DIFFER STAY VISIBLE.  NO SMOOTHING OF THE VIEW LABELS in this call (off by
 *   default: see sfmba_mesh_texture_smooth in the next section).  NO CHART MERGING: THE ATLAS SPENDS (S + 1) S / 2 TEXELS ON EVERY
 *   TRIANGLE, HOWEVER SMALL.
 *
 * sfmba_mesh_texture_size
 *   *width = W and *height = H of the layout above; SFMBA_ERR_INVALID_ARG for what the call refuses about n_triangles, S, B, W and H.
 *
 *   SFMBA_ERR_INVALID_ARG (nothing written): whatever the fuse refuses about images, sizes, K and P; a negative or >= 2^31 count;
 *                 a triangle index outside 0 .. n_vertices-1 (found on the device, before anything is written); S outside 3..64;
 *                 B < 1; W or H above 16384; occl_tol not finite or < 0; min_area < 0; a NULL atlas, uv, view or n_textured (width
 *                 or height for the size); a NULL xyz with n_vertices > 0, tri with n_triangles > 0, depth with n_images > 0.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_mesh_texture_size(int64_t n_triangles, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/, int32_t* width,
                int32_t* height);
SFMBA_API int sfmba_mesh_texture(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/, float occl_tol,
                int64_t min_area /*in (1/16 px)^2, doubled; >= 0*/, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/,
                unsigned char* atlas /*[H][W][3] BGR*/, float* uv /*[n_triangles][3][2]*/, int32_t* view /*[n_triangles]*/,
                int64_t* score /*[n_triangles] or NULL*/, int64_t* n_textured);

/* ---- smoothing the view labels: the K best views, the adjacency, score diffusion and a Potts relaxation (SfM::textureMesh) --------
 * sfmba_mesh_texture chooses a view per triangle with no regard for its neighbours: where two views see a surface about equally large,
 * the largest-area rule flips between them on noise, and every flip is a seam in the atlas.  The calls of this section choose the labels
 * TOGETHER.  OFF BY DEFAULT: nothing above changes.  Like the texture call THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S, and it is stated
 * so that the device is held BIT FOR BIT to a CPU restatement (tests/label_oracle.py).  The projection arithmetic is exactly the texture
 * call's (a view's candidate flag, score and eligibility as "view choice" above states them) and is not restated; EVERYTHING ELSE IS
 * INTEGER ARITHMETIC (csrc/label_math.h).  The only atomics are integer adds on the statistics, whose result does not depend on order.
 * T = n_triangles, K = n_candidates.  Every call that sorts edges needs 3 T < 2^31.
 *
 * sfmba_mesh_view_candidates
 *   the mesh (xyz, tri), the views and occl_tol, min_area of sfmba_mesh_texture, and K in 1..8.  Per triangle the K ELIGIBLE views of
 *   largest score, in descending score, TIES TO THE LOWER VIEW INDEX: cand_view int32 [T][K], cand_score int64 [T][K]; unused entries
 *   are -1 and 0 and follow the used ones.  Rank 0 equals view[t] / score[t] of sfmba_mesh_texture bit for bit.  A triangle with a
 *   repeated index or a non-finite coordinate gets no candidate.  Every score lies in 1 .. 2^37 - 1 (|su|, |sv| < 2^18).
 *
 * sfmba_mesh_adjacency
 *   adj int32 [T][3].  Edge q of triangle t joins tri[t][q] and tri[t][(q + 1) % 3]; its key is (min << 32) | max of the two indices
 *   (which must be >= 0; no vertex is read, so there is no upper limit).  A triangle with a repeated index contributes no edge, and its
 *   three adj entries are -1.  An edge whose key occurs EXACTLY TWICE links its two triangles: adj[t][q] of either is the other.  A key
 *   that occurs once is OPEN; a key that occurs three or more times is NON-MANIFOLD; every adj entry on such an edge is -1.  Two
 *   triangles on the same three vertices are linked three times.  *n_pairs, *n_open_edges, *n_nonmanifold_edges count the keys of each
 *   kind.  (Implementation: the keys, one stable radix sort with the value 3 t + q, one lane per sorted entry.)
 *
 * sfmba_mesh_view_smooth
 *   cand_view, cand_score [T][K] as the candidates call writes them (each row: scores in 1 .. 2^37 - 1 in descending order with views in
 *   0 .. n_images-1, then -1 and 0; anything else is refused), adj [T][3] with entries in -1 .. T-1, rings r in 0..8, penalty p in
 *   0..65535, max_passes in 0..10000.  Writes view int32 [T] and stats int64 [8].  "n in adj(t)" runs over the three ENTRIES of adj[t]
 *   that are >= 0: a triangle linked twice to the same neighbour counts it twice.
 *   1 diffusion   s^0 = cand_score.  For i = 0 .. r-1 and every entry with cand_view[t][k] >= 0:
 *                 s^{i+1}[t][k] = s^i[t][k] + sum over n in adj(t) of look(n, cand_view[t][k]), where look is s^i[n][j] for the FIRST j
 *                 with cand_view[n][j] equal to that view, and 0 if n does not list it.  Entries with cand_view = -1 stay 0.  Every ring
 *                 reads only the ring before (a Jacobi update).  A sum has at most four terms, so s^r < 4^8 2^37 = 2^53: int64 holds it.
 *   2 start       rank[t] = the k of the largest s^r[t][k] among the entries with cand_view[t][k] >= 0, THE LOWEST k ON A TIE;
 *                 view[t] = cand_view[t][rank[t]]; a triangle without a candidate has view -1 for good, never moves and pulls on nobody.
 *                 With r = 0 the start is rank 0, the texture call's label.
 *   3 data term   from the ORIGINAL scores: D[t][k] = floor(1024 (cand_score[t][0] - cand_score[t][k]) / cand_score[t][0]), 0..1023.
 *   4 a pass      for a triangle with a candidate and every k with cand_view[t][k] >= 0:
 *                 e[t][k] = D[t][k] + p #{n in adj(t): view[n] >= 0 and view[n] != cand_view[t][k]}; k* = the lowest k of least e;
 *                 gain[t] = e[t][rank[t]] - e[t][k*] (>= 0; 0 for a triangle without a candidate).  t MOVES (rank[t] = k*, view[t] =
 *                 cand_view[t][k*]) iff gain[t] > 0 and, for every n in adj(t), gain[t] > gain[n] or (gain[t] == gain[n] and t < n).
 *                 ALL GAINS COME FROM THE LABELS BEFORE THE PASS.  With a symmetric adj (the adjacency call's) the movers of a pass are
 *                 pairwise non-adjacent and the energy E = sum_t D[t][rank[t]] + p #{pairs with both views >= 0 and different} falls
 *                 by exactly the sum of the movers' gains.  Passes run until one moves nothing or max_passes have run.
 *   5 stats       a PAIR is an entry n = adj[t][q] with t < n.  stats[0] = E after the start, [1] = E at the end; the pairs with both
 *                 views >= 0 and different [2] under rank 0, [3] after the start, [4] at the end; [5] the pairs with exactly one view
 *                 -1 (a frontier between textured and untextured, which no pass can move: not a seam between two photographs);
 *                 [6] the moves of all passes; [7] the passes in which something moved.
 *   A triangle never gets a view that is not one of its own eligible candidates.
 *
 * sfmba_mesh_texture_from_views
 *   sfmba_mesh_texture with view [T] as an INPUT: each entry is -1 or in 0 .. n_images-1 (anything else is refused, found on the device
 *   before anything is written).  The same layout, texels, uv and atlas; no depth map, occl_tol or min_area, since nothing is tested.
 *   *n_textured is the number of entries >= 0.
 *
 * sfmba_mesh_texture_smooth
 *   candidates, adjacency, smoothing and the texture call's raster in ONE call, everything staying on the device.  It equals the
 *   composition of the four calls above byte for byte: view and stats of the smoothing, score[t] = cand_score[t][rank[t]] (0 without a
 *   candidate; may be NULL), atlas, uv and *n_textured of from_views.  With rings = 0 and max_passes = 0 it equals sfmba_mesh_texture
 *   byte for byte in atlas, uv, view, score and n_textured.
 *
 *   OUT OF SCOPE: chart merging; letting a triangle below the area floor borrow a neighbour's view; any
 *   optimiser stronger than this local one (no graph cut, no message passing).
 *   SFMBA_ERR_INVALID_ARG (nothing written): what sfmba_mesh_texture refuses about the arguments a call shares with it; K outside 1..8;
 *                 rings outside 0..8; penalty outside 0..65535; max_passes outside 0..10000; 3 T >= 2^31; a negative index
 *                 (adjacency); an adj entry outside -1 .. T-1; a cand_view outside -1 .. n_images-1 or a row that is no candidate
 *                 list; a view outside -1 .. n_images-1 (from_views, found on the device); a NULL output, or a NULL input array with
 *                 T > 0.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_mesh_view_candidates(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, int64_t n_triangles,
                const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr, const unsigned char* pixels,
                const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/, const float* P /*[n_images][12]*/,
                const float* const* depth /*[n_images], each NULL or [h][w]*/, float occl_tol, int64_t min_area, int n_candidates /*1..8*/,
                int32_t* cand_view /*[n_triangles][n_candidates]*/, int64_t* cand_score /*[n_triangles][n_candidates]*/);
SFMBA_API int sfmba_mesh_adjacency(int device, int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int32_t* adj /*[n_triangles][3]*/,
                int64_t* n_pairs, int64_t* n_open_edges, int64_t* n_nonmanifold_edges);
SFMBA_API int sfmba_mesh_view_smooth(int device, int64_t n_triangles, int n_images, int n_candidates /*1..8*/,
                const int32_t* cand_view /*[n_triangles][n_candidates]*/, const int64_t* cand_score /*[n_triangles][n_candidates]*/,
                const int32_t* adj /*[n_triangles][3]*/, int rings /*0..8*/, int penalty /*0..65535*/, int max_passes /*0..10000*/,
                int32_t* view /*[n_triangles]*/, int64_t* stats /*[8]*/);
SFMBA_API int sfmba_mesh_texture_from_views(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/,
                const int32_t* view /*[n_triangles], each -1 or an image*/, unsigned char* atlas /*[H][W][3] BGR*/,
                float* uv /*[n_triangles][3][2]*/, int64_t* n_textured);
SFMBA_API int sfmba_mesh_texture_smooth(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/, float occl_tol,
                int64_t min_area, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/, int n_candidates /*1..8*/, int rings /*0..8*/,
                int penalty /*0..65535*/, int max_passes /*0..10000*/, unsigned char* atlas /*[H][W][3] BGR*/,
                float* uv /*[n_triangles][3][2]*/, int32_t* view /*[n_triangles]*/, int64_t* score /*[n_triangles] or NULL*/,
                int64_t* n_textured, int64_t* stats /*[8]*/);

/* ---- levelling the colours across seams: a node per (vertex, view), additive offsets by integer diffusion (SfM::textureMesh) --------
 * Where two triangles take their texels from different photographs, the difference in exposure and vignetting shows as a step at the
 * shared edge.  The calls of this section give every (vertex, view) pair an additive colour offset: the offsets of one vertex in two
 * views close the gap between the two photographs, the offsets within one view vary smoothly over the mesh, and the raster interpolates
 * the offset across each triangle's patch (global seam levelling after Lempitsky & Ivanov and Waechter et al., by Jacobi passes).
 * OFF BY DEFAULT: nothing above changes.  THE CONTRACT IS OUR OWN AND EQUALS NOBODY'S, and it is stated so that the device is held BIT
 * FOR BIT to a CPU restatement (tests/colour_oracle.py).  Past the fixed-point image coordinate of the texture call EVERYTHING IS
 * INTEGER ARITHMETIC (csrc/colour_math.h) and every division is a FLOOR division.  The only atomic is an integer add on the count of
 * clamped texels.  T = n_triangles; a sum written a + b + c is ((a + b) + c).  Every call of this section needs 3 T < 2^31.
 *
 * sfmba_mesh_colour_nodes
 *   the mesh (xyz, tri), the views exactly as sfmba_mesh_texture_from_views takes them, view [T] GIVEN (each entry -1 or an image
 *   index) and a sample radius r in 0..2.  A triangle CONTRIBUTES iff view[t] >= 0, it has no repeated index and its three vertices are
 *   finite; it names the three keys (tri[t][q] << 32) | view[t].  A NODE is a distinct key; nodes are numbered in ascending key order.
 *   Outputs: *n_nodes; node_vertex, node_view int32 [3 T] and seen uint8 [3 T], F int32 [3 T][3], of which the first n_nodes entries
 *   are written (the caller provides 3 T); node_of int32 [T][3], -1 -1 -1 for a triangle that does not contribute.
 *   The colour of a node (v, l): X = the doubles of the vertex's floats; the texture call's texel rule gives (su, sv) in view l; where it
 *   gives none (q_2 <= 0 or a NaN) the node is BLIND: seen = 0, F = 0.  Otherwise seen = 1 and, with n = (2 r + 1)^2, per channel c
 *   SUM = the sum of the 12-bit samples at (clamp(su + 16 dx, 0, 16 (w - 1)), clamp(sv + 16 dy, 0, 16 (h - 1))) over dx, dy in -r..r
 *   and F_c = floor((32 SUM + n) / (2 n)): the mean sample in 1/256 grey level, 0..65280.  A gray image gives three equal channels.
 *   (Implementation: the keys, one stable radix sort with the value 3 t + q, head flags and an exclusive sum.)
 *
 * sfmba_mesh_colour_level
 *   PURE INTEGER: it reads no pixel and no coordinate.  Inputs: n_nodes, node_vertex [n_nodes] NON-DECREASING, seen [n_nodes] (not 0:
 *   seeing), F [n_nodes][3] each in 0..65280, node_of [T][3] with every row all -1 or all in 0 .. n_nodes-1, a seam weight w in 1..256
 *   and passes N in 0..1024.  Outputs: g int32 [n_nodes][3] in 1/256 grey level and stats int64 [8].
 *   g^0 = 0.  A blind node keeps g = 0, belongs to no sibling set and is nobody's link.  sib(n) is the seeing nodes with n's
 *   node_vertex, n INCLUDED; k = |sib(n)|.  The LINKS of n are, for every entry node_of[t][q] = n, the two other entries of that row
 *   that are seeing nodes: an interior edge of one view counts twice and a border edge once, which is intended.
 *   One pass, for every seeing node n and channel c: A = sum over m in sib(n) of ((F_m + g^i_m) - F_n) and a = k if k >= 2, else
 *   A = a = 0; B = the sum of g^i_u over the links of n and b their number; den = w a + b, num = w A + B.  If den = 0,
 *   g^{i+1}_n = g^i_n; otherwise g^{i+1}_n = clamp(floor((2 num + den) / (2 den)), -65280, 65280).  Every pass reads only the pass
 *   before (Jacobi, two buffers); exactly N passes run: no convergence test.  k <= n_images, |F + g| < 2^18, w <= 2^8: int64 holds
 *   every sum with room to spare.  With the node in its own sibling set the spread at a seam falls monotonically with the passes.
 *   stats: [0] nodes, [1] blind nodes, [2] SEAM VERTICES (vertices with k >= 2), [3] the sum over seam vertices and channels of
 *   (max - min of F over the siblings), [4] the same of F + g^N, [5] the largest |g^N|, [6] 0 (see the adjust call), [7] N.
 *
 * sfmba_mesh_texture_levelled
 *   sfmba_mesh_texture_from_views plus node_of [T][3], g [n_nodes][3] (each in -65280..65280) and n_nodes: the same layout, uv and
 *   fallback.  A texel that is SAMPLED takes per channel G = (wA g_A + wB g_B) + wC g_C with the texel's own integer weights (the
 *   least is -1) and the offsets of the nodes node_of[t][0..2] (a row of -1: G = 0), and
 *   texel = clamp(floor((16 (S - 2) s12 + G + 128 (S - 2)) / (256 (S - 2))), 0, 255).  With G = 0 this is (s12 + 8) >> 4, the texture
 *   call's texel.  FALLBACK TEXELS ARE NEVER ADJUSTED.  Extra outputs: *n_textured, and *n_clamped = the texels for which the clamp
 *   changed at least one channel.
 *
 * sfmba_mesh_texture_adjust
 *   the arguments of sfmba_mesh_texture_smooth, then sample_radius, seam_weight, level_passes and level_stats int64 [8]: the labels
 *   first (with rings = 0 and max_passes = 0 they are the plain rule's), then nodes, offsets and the levelled raster, everything staying
 *   on the device.  It equals the composition of the separate calls byte for byte; level_stats holds the level call's statistics
 *   with [6] = n_clamped.  With level_passes = 0 it equals sfmba_mesh_texture_smooth byte for byte in atlas, uv, view, score, n_textured
 *   and stats.
 *
 *   OUT OF SCOPE: per-view gain or gamma estimation (the offsets are additive and local); Poisson blending of patch interiors; colour
 *   statistics sampled along edges rather than at vertices; chart merging.
 *   SFMBA_ERR_INVALID_ARG (nothing written): everything the calls of the shared arguments refuse; r outside 0..2; w outside 1..256;
 *                 passes outside 0..1024; 3 T >= 2^31; a node_of entry outside -1 .. n_nodes-1 or a row that is partly -1; a
 *                 decreasing node_vertex; an F outside 0..65280; a g outside -65280..65280 (levelled); a view outside
 *                 -1 .. n_images-1 (found on the device, before anything is written); a NULL output, or a NULL input array with a
 *                 positive count.
 *   Host pointers in and out, synchronous, deterministic.  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_mesh_colour_nodes(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, int64_t n_triangles,
                const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr, const unsigned char* pixels,
                const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/, const float* P /*[n_images][12]*/,
                const int32_t* view /*[n_triangles], each -1 or an image*/, int sample_radius /*0..2*/, int64_t* n_nodes,
                int32_t* node_vertex /*[3 n_triangles]*/, int32_t* node_view /*[3 n_triangles]*/, int32_t* node_of /*[n_triangles][3]*/,
                unsigned char* seen /*[3 n_triangles]*/, int32_t* F /*[3 n_triangles][3]*/);
SFMBA_API int sfmba_mesh_colour_level(int device, int64_t n_nodes, const int32_t* node_vertex /*[n_nodes]*/, const unsigned char* seen /*[n_nodes]*/,
                const int32_t* F /*[n_nodes][3]*/, int64_t n_triangles, const int32_t* node_of /*[n_triangles][3]*/,
                int seam_weight /*1..256*/, int passes /*0..1024*/, int32_t* g /*[n_nodes][3]*/, int64_t* stats /*[8]*/);
SFMBA_API int sfmba_mesh_texture_levelled(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/,
                const int32_t* view /*[n_triangles], each -1 or an image*/, const int32_t* node_of /*[n_triangles][3]*/,
                const int32_t* g /*[n_nodes][3]*/, int64_t n_nodes, unsigned char* atlas /*[H][W][3] BGR*/,
                float* uv /*[n_triangles][3][2]*/, int64_t* n_textured, int64_t* n_clamped);
SFMBA_API int sfmba_mesh_texture_adjust(int device, int64_t n_vertices, const float* xyz /*[n_vertices][3]*/, const unsigned char* bgr /*or NULL*/,
                int64_t n_triangles, const int32_t* tri /*[n_triangles][3]*/, int n_images, const int64_t* img_ptr,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels, const float* K /*[9]*/,
                const float* P /*[n_images][12]*/, const float* const* depth /*[n_images], each NULL or [h][w]*/, float occl_tol,
                int64_t min_area, int patch /*S, 3..64*/, int blocks_per_row /*B >= 1*/, int n_candidates /*1..8*/, int rings /*0..8*/,
                int penalty /*0..65535*/, int max_passes /*0..10000*/, unsigned char* atlas /*[H][W][3] BGR*/,
                float* uv /*[n_triangles][3][2]*/, int32_t* view /*[n_triangles]*/, int64_t* score /*[n_triangles] or NULL*/,
                int64_t* n_textured, int64_t* stats /*[8]*/, int sample_radius /*0..2*/, int seam_weight /*1..256*/,
                int level_passes /*0..1024*/, int64_t* level_stats /*[8]*/);

/* ---- matching by optical flow: pyramidal Lucas-Kanade and the snap to key points (SfMFeatureMatching::createFlowMatchMatrix) -----
 * The reference's legacy tree matched video-like input without descriptors (legacy/SfMToyLib_Old/OFFeatureMatcher.cpp): it tracked
 * the key points of image i into image j with gpu::PyrLKOpticalFlow::sparse, snapped every flow end point to a key point of j
 * within 2 px, applied a 0.7 ratio test and dropped duplicates in query order.  Here a list of image pairs is tracked in one call and
 * snapped in a second.  THE TRACKER'S CONTRACT IS OUR OWN AND EQUALS NOBODY'S (OpenCV's tracker is float arithmetic in an unstated
 * order); like the dense unit's it is stated so that the device is held BIT FOR BIT to a CPU restatement (tests/flow_oracle.py):
 * integer-exact samples at 1/16 px, exact window sums, a handful of fp64 operations, EVERY ONE ROUNDED ON ITS OWN (no fused
 * multiply-add anywhere; csrc/flow_math.h switches the compiler's contraction off).
 *
 * sfmba_flow_track
 *   images        as sfmba_orb_extract takes them, with the same BGR -> gray rule.  Images may differ in size.
 *   pairs         pair p tracks from image pair_src[p] into image pair_dst[p] (src == dst is allowed) and owns the points
 *                 pt_ptr[p] .. pt_ptr[p+1]-1 of pts float [.][2]: finite coordinates (x, y) in the source image.
 *                 Shared: n_levels L in 1..8, radius r in 1..10 (the window holds n = (2r+1)^2 pixels), max_iters in 1..64,
 *                 min_eig >= 0 (a finite float).
 *   pyramid       per image, once per group of pairs that names it: level 0 is the gray image; level l+1 has the size
 *                 ((w+1)>>1, (h+1)>>1) and its pixel (x, y) is (sum_ij k_i k_j I_l(clamp(2x+i-2), clamp(2y+j-2)) + 128) >> 8 with
 *                 k = 1 4 6 4 1, i, j = 0..4, coordinates clamped to the image: exact integer arithmetic.
 *   sampler       S(I, su, sv) clamps su to [0, 16 (w-1)] and sv to [0, 16 (h-1)] and then applies the 1/16 px bilinear rule of
 *                 sfmba_depth_sweep's sample: a 12-bit integer 0..4080, defined for every (su, sv).
 *   per point     from level L-1 down to level 0.  The displacement dq is an integer 2-vector in 1/16 px of the current level; it
 *                 starts at 0 and doubles on each step down a level.  At level l, per coordinate, c = floor(16 (x / 2^l) + 0.5)
 *                 with x converted to double exactly (the scaling is exact; c saturates at +-2^28, which no output can tell from
 *                 the exact value: such a centre reads the clamped edge wherever dq takes it and never has status 1).
 *                 T(i, j) = S(src_l, c + 16 (i, j)) for i, j in -r-1 .. r+1; over i, j in -r .. r:
 *                 gx = T(i+1, j) - T(i-1, j), gy = T(i, j+1) - T(i, j-1), Gxx = sum gx^2, Gyy = sum gy^2, Gxy = sum gx gy, exact
 *                 in int64 (each below 441 * 4080^2 = 7341062400 < 2^33).  In fp64: det = (double)Gxx (double)Gyy -
 *                 (double)Gxy (double)Gxy, df = (double)(Gxx - Gyy), lam = ((double)(Gxx + Gyy) - sqrt(df df + 4.0 ((double)Gxy
 *                 (double)Gxy))) 0.5.  The level is TRACKABLE iff det > 0 and lam >= ((double)min_eig (double)n) 1024.0 --
 *                 1024 = (2 * 16)^2 is the scale of a central difference of x16 samples, so min_eig is a per-pixel squared gradient
 *                 in (gray levels / px)^2.  A level that is not trackable carries dq on unchanged.
 *   iteration     on a trackable level, at most max_iters times: J(i, j) = S(dst_l, c + dq + 16 (i, j)), D = T - J,
 *                 bx = sum D gx, by = sum D gy (exact int64); nx = (double)Gyy (double)bx - (double)Gxy (double)by,
 *                 ny = (double)Gxx (double)by - (double)Gxy (double)bx; sx = floor((32.0 nx) / det + 0.5) clamped to +-16 r, sy
 *                 likewise (32 = 16 units per pixel times 2 for the central difference).  If sx == 0 and sy == 0 the level ends
 *                 (that evaluation counts as an iteration), otherwise dq += (sx, sy).  No oscillation rule: a point may run to
 *                 max_iters on a two-cycle of +-1/16 px.
 *   outputs       per point, in input order: next float [.][2] = (float)((double)x + (double)dq_x / 16.0), y likewise (dq of
 *                 level 0); status uint8 = 1 iff level 0 was trackable and c_0 + dq lies in [0, 16 (w_dst-1)] x [0, 16 (h_dst-1)],
 *                 tested unclamped; err float = (float)((double)(sum |T - J|) / (16.0 (double)n)) over the window at level 0 with
 *                 the final dq (one more evaluation after the last step) when level 0 was trackable, 0 otherwise.
 *   debug         each may be NULL.  dbg_G int64 [.][L][3] = Gxx, Gyy, Gxy and dbg_state int32 [.][L][4] = the trackable flag, the
 *                 iterations run and the dq leaving the level, per (point, level l; l = 0 is the finest).  dbg_pyramid uint8: image
 *                 i's levels 0 .. L-1 back to back (each row-major), images in order; only images that a pair names are written.
 *   SFMBA_ERR_INVALID_ARG (nothing written): whatever sfmba_orb_extract refuses about images; n_levels, radius, max_iters or
 *                 min_eig (NaN included) outside the ranges above; a pair index out of range; a pt_ptr that does not start at 0 or
 *                 decreases; a point coordinate that is not finite; 2^31 or more points in one call.
 *   Host pointers in and out, synchronous.  Deterministic; pairs go to the device in consecutive groups under a fixed scratch bound
 *   (512 MiB of images, pyramids and per-point arrays) and the result does not depend on the grouping: a batch equals the
 *   concatenation of single-pair calls.
 *   First choices that nobody has tuned: L = 4, r = 7, max_iters = 20, min_eig = 1.
 *
 * sfmba_flow_match
 *   inputs        per pair p the tracker's next, status and err with the same pt_ptr (queries); per image i its key points
 *                 kp_xy[kp_ptr[i] .. kp_ptr[i+1]-1] float [.][2], fewer than 2^22 per image; pair p's train set is that of image
 *                 pair_dst[p].  max_err (finite), radius > 0 (finite), ratio > 0 (finite).  The reference's values: 12, 2, 0.7.
 *   eligible      query q iff status[q] != 0 and err[q] < max_err.
 *   distance      s(q, j) = dx dx + dy dy with dx = (double)next_x - (double)kp_x, dy likewise; j is IN RANGE iff
 *                 s <= (double)radius (double)radius.
 *   candidate     none in range: no candidate.  Exactly one: that one.  Two or more: of the two smallest (s, j) in lexicographic
 *                 order the best is the candidate iff sqrt(s_best) < ratio sqrt(s_second), with correctly rounded fp64 roots -- so
 *                 two coincident key points give 0 < 0 and the query is dropped.
 *   duplicates    among the candidates of a pair that name the same train index the lowest q wins (the reference's
 *                 found_in_imgpts_j set, walked in query order; on the device an integer atomicMin per train key point, which does
 *                 not depend on the arrival order).
 *   output        (query_idx = q - pt_ptr[p], train_idx = j, distance = (float)sqrt(s_best)) in ascending q within a pair, with the
 *                 pair_ptr CSR, the capacity protocol and *total of sfmba_match_features.
 *   SFMBA_ERR_INVALID_ARG (nothing written): max_err, radius or ratio not finite, radius or ratio <= 0; a pair index out of range;
 *                 a pt_ptr or kp_ptr that does not start at 0 or decreases; 2^22 or more key points in one image; 2^31 or more
 *                 queries in one call.
 *   Host pointers in and out, synchronous, deterministic.  The call is one batch: 45 bytes of device memory per query and 4 per (pair,
 *   train key point).  SFMBA_ABI_VERSION stays 6: adding symbols is backward compatible.
 */
SFMBA_API int sfmba_flow_track(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* pixels, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/,
                int n_pairs, const int32_t* pair_src /*[n_pairs]*/, const int32_t* pair_dst /*[n_pairs]*/,
                const int64_t* pt_ptr /*[n_pairs+1]*/, const float* pts /*[pt_ptr[n_pairs]][2]*/, int n_levels /*1..8*/,
                int radius /*1..10*/, int max_iters /*1..64*/, float min_eig /*>= 0*/, float* next /*[.][2]*/,
                unsigned char* status /*[.]*/, float* err /*[.]*/, int64_t* dbg_G /*[.][n_levels][3] or NULL*/,
                int32_t* dbg_state /*[.][n_levels][4] or NULL*/, unsigned char* dbg_pyramid /*or NULL*/);
SFMBA_API int sfmba_flow_match(int device, int n_images, const int64_t* kp_ptr /*[n_images+1]*/, const float* kp_xy /*[kp_ptr[n_images]][2]*/,
                int n_pairs, const int32_t* pair_dst /*[n_pairs]*/, const int64_t* pt_ptr /*[n_pairs+1]*/, const float* next /*[.][2]*/,
                const unsigned char* status /*[.]*/, const float* err /*[.]*/, float max_err, float radius, double ratio,
                int64_t* pair_ptr /*[n_pairs+1]*/, int32_t* query_idx, int32_t* train_idx, float* distance /*or NULL*/, int64_t cap,
                int64_t* total);

/* ---- reading photographs: baseline JPEG decode and bilinear resize (SfM::setImagesDirectory) -----------------------------------
 * The reference reads every image with imread and shrinks it with resize(..., Size(), f, f) (SfMToyLib/SfM.cpp:125-129).  Here a
 * whole list of files is decoded, and a whole list of images resized, in one call each.  THE CONTRACT IS INTEGER-EXACT: the decode
 * equals libjpeg's default decode (integer "islow" inverse DCT, triangle chroma upsampling) of a baseline file bit for bit, the
 * resize is our own fixed-point statement of cv::resize(..., INTER_LINEAR)'s sampling positions, and the device is held BIT FOR BIT
 * to a CPU restatement of both (tests/jpeg_oracle.py).
 *
 *   files         file i owns bytes file_ptr[i] .. file_ptr[i+1]-1 of bytes.
 *   accepted      baseline sequential DCT (SOF0), 8-bit samples, Huffman coding, 8-bit quantisation tables, one component (gray) or
 *                 three (Y, Cb, Cr) in one interleaved scan with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, any restart
 *                 interval, width and height in 1..16384.  APPn and COM segments are skipped; EXIF ORIENTATION IS IGNORED.
 *   status        per image, never a failure of the call: SFMBA_IMAGE_UNSUPPORTED for a well-formed file outside that scope
 *                 (progressive, arithmetic coding, 12-bit samples, 16-bit quantisation tables, two or four components, other
 *                 sampling factors, several scans, a side above 16384) and never a guess at its pixels; SFMBA_IMAGE_CORRUPT for a
 *                 file that breaks its own syntax (truncated, a segment length past the end of the file, a missing table, a
 *                 Huffman code that is not in the table, a coefficient index past 63, a DC value outside int16, zero dimensions,
 *                 a missing restart marker).  Such an image has no pixels (out_ptr[i+1] == out_ptr[i]) and the fields of its
 *                 sfmba_image_info besides status are 0; the other images of the batch are decoded normally.
 *   host          headers and entropy decoding run on the host with at most min(n_images, 16) threads and yield int16 coefficients
 *                 in natural order plus quantisers and geometry; the device never sees file bytes.
 *   inverse DCT   per 8 x 8 block, coefficient times quantiser, then the two-pass integer transform with CONST_BITS = 13 and
 *                 PASS1_BITS = 2 and the constants 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172: columns
 *                 first with DESCALE(x, 11), then rows with DESCALE(x, 18), DESCALE(x, n) = (x + (1 << (n-1))) >> n; the sample is
 *                 clamp(v + 128, 0, 255).  All intermediates are 32-bit two's complement with wrap-around (formed unsigned).
 *   chroma        a component is ceil(W h / hmax) x ceil(H v / vmax) samples; the MCU padding beyond that is never read.
 *                 2x1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, the first and the last
 *                 output of a row copy the edge sample.  2x2: s[i] = 3 near[i] + far[i] with far the row above for the upper
 *                 output row and the row below for the lower one (at the top and bottom the component's own edge row is repeated);
 *                 out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, at the edges (4 s + 8) >> 4 and
 *                 (4 s + 7) >> 4.
 *   colour        with cb, cr centred on 128: R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16),
 *                 G = Y + ((-22554 cb - 46802 cr + 32768) >> 16) (arithmetic shifts), each clamped to 0..255.  Three components
 *                 come back as B, G, R interleaved (CV_8UC3), one component as it is; rows tight.
 *   resize        one factor for both axes, f = (double)factor.  ow = lrint(w f), oh = lrint(h f) (round-half-even); inv = 1 / f.
 *                 Per output column x (rows likewise): fx = (x + 0.5) inv - 0.5, sx = floor(fx), a = fx - sx, or a = 0 where
 *                 sx < 0 or sx >= w - 1 with the index clamped into 0..w-1; w1 = lrint(2048 a), w0 = 2048 - w1; the second sample
 *                 is at min(sx + 1, w - 1).  The tables are built on the host in double.  Every channel:
 *                 out = (wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) + (1 << 21)) >> 22, which fits 32 bits and lies within
 *                 1 level of the exact bilinear value.
 *
 * sfmba_jpeg_info: headers only (up to the start of the scan), host only, no device needed; info [n_images].  A file whose headers
 *   are in order reports SFMBA_IMAGE_OK here even when its scan data will prove corrupt in sfmba_jpeg_decode -- except that a frame
 *   of more than 4 blocks of 8 x 8 per byte left in the file is SFMBA_IMAGE_CORRUPT already (a block takes at least 2 bits), so no
 *   array is ever sized from a frame that its file cannot hold.
 * sfmba_resized_size: ow, oh of the resize rule; SFMBA_ERR_INVALID_ARG when factor is not finite and > 0 or a result lies outside
 *   1..16384.  Host only.
 * sfmba_jpeg_decode: info [n_images] (the final status), out_ptr [n_images + 1] (byte offsets into out), out [cap].  With
 *   factor != 1 every image is resized before its pixels leave the device; the result equals factor = 1 followed by
 *   sfmba_resize_images byte for byte, and info then still reports the size of the file's own image.
 * sfmba_resize_images: image i owns bytes img_ptr[i] .. img_ptr[i+1]-1 of px, height[i] rows of width[i] * channels bytes;
 *   channels is 1 or 3.
 * Both device calls: host pointers in and out, synchronous; *total receives the number of bytes; SFMBA_ERR_CAPACITY (info, out_ptr
 * and *total valid, out untouched) if cap < *total.  SFMBA_ERR_INVALID_ARG (nothing written) for a factor that is not finite and
 * > 0 or that gives an image a side outside 1..16384 (judged from the headers, before any scan is decoded), a source side outside 1..16384, an img_ptr that does not agree with the
 * sizes, a decreasing file_ptr.  Deterministic: a batch equals the concatenation of single-image calls (images go to the device in
 * consecutive groups under a fixed scratch bound).  SFMBA_ABI_VERSION stays 6: adding a symbol is backward compatible.
 */
enum { SFMBA_IMAGE_OK = 0, SFMBA_IMAGE_UNSUPPORTED = 1, SFMBA_IMAGE_CORRUPT = 2 };
typedef struct sfmba_image_info { int status; int width, height, channels; int h_samp, v_samp; int restart_interval; } sfmba_image_info;
SFMBA_API int sfmba_jpeg_info(int n_images, const int64_t* file_ptr /*[n_images+1], byte offsets*/, const unsigned char* bytes,
                sfmba_image_info* info /*[n_images]*/);
SFMBA_API int sfmba_resized_size(int width, int height, float factor, int32_t* out_width, int32_t* out_height);
SFMBA_API int sfmba_jpeg_decode(int device, int n_images, const int64_t* file_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* bytes, float factor, sfmba_image_info* info /*[n_images]*/, int64_t* out_ptr /*[n_images+1]*/,
                unsigned char* out /*[cap]*/, int64_t cap, int64_t* total);
SFMBA_API int sfmba_resize_images(int device, int n_images, const int64_t* img_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* px, const int32_t* width, const int32_t* height, int channels /*1 gray, 3 BGR*/, float factor,
                int64_t* out_ptr /*[n_images+1]*/, unsigned char* out /*[cap]*/, int64_t cap, int64_t* total);

/* ---- reading PNG files: inflate on the host, unfilter and unpack on the device (SfM::setImagesDirectory) --------------------------
 * The reference's setImagesDirectory takes "jpg and png" (SfMToyLib/SfM.h, SfM.cpp:98-139).  Call conventions, status values, groups,
 * SFMBA_ERR_CAPACITY and SFMBA_ERR_INVALID_ARG are exactly those of sfmba_jpeg_info / sfmba_jpeg_decode above; the resize is the same
 * kernel and tables.  THE CONTRACT IS INTEGER-EXACT, our own statement, and the device is held BIT FOR BIT to a CPU restatement
 * (tests/png_oracle.py); it equals Pillow's decode (convert("L" / "RGB"), >> 8 for 16-bit gray) for all 15 accepted pairs.
 *
 *   accepted      colour type 0 at depth 1, 2, 4, 8, 16; 2 at 8, 16; 3 at 1, 2, 4, 8; 4 at 8, 16; 6 at 8, 16; compression 0, filter
 *                 method 0, no interlace, width and height in 1..16384; any number of IDAT chunks, consecutive.
 *   chunks        every chunk's CRC is checked; ancillary chunks (tRNS, gAMA, sRGB, tEXt, ...) are skipped: NO GAMMA AND NO
 *                 TRANSPARENCY PROCESSING.  Bytes after IEND, and bytes of the zlib stream after its Adler-32, are ignored.
 *   status        per image, never a failure of the call.  SFMBA_IMAGE_UNSUPPORTED for a well-formed file outside that scope: Adam7
 *                 interlace, a side above 16384, a critical chunk other than IHDR, PLTE, IDAT, IEND.  SFMBA_IMAGE_CORRUPT for a bad
 *                 signature, a bad CRC, a chunk length past the end of the file, IHDR missing, not first, repeated or of wrong
 *                 length, an illegal depth / colour type pair, a compression, filter or interlace method that does not exist, zero
 *                 dimensions, colour type 3 without PLTE before IDAT, a PLTE that is empty, repeated, placed after IDAT, not a
 *                 multiple of 3 long or of more than 256 entries, no IDAT, IDAT chunks that are not consecutive, IEND missing; a zlib
 *                 header that is not deflate with a window of at most 32 K, that names a preset dictionary or whose check bits are
 *                 wrong; an invalid deflate stream (reserved block type, stored-block length check, an over-subscribed or incomplete
 *                 code -- a single code of length 1 and, for distances, no code at all are complete enough, as in zlib --, a code not
 *                 in the table, a distance before the start of the output, input that ends early); an Adler-32 mismatch; an inflated
 *                 length other than exactly height x (1 + rowbytes); a filter-type byte above 4 (checked by the host on the inflated
 *                 stream).  Such an image has no pixels and the fields of its sfmba_png_info besides status are 0; the other images
 *                 of the batch are decoded normally.
 *   size gate     an image whose height x (1 + rowbytes) exceeds 1032 x the total of IDAT bytes + 64 is SFMBA_IMAGE_CORRUPT before
 *                 anything is sized from it: a deflate stream cannot expand further.
 *   host          chunk walk, CRC-32, zlib wrapper and the project's own inflate (stored, fixed and dynamic blocks, table-driven,
 *                 into a buffer of exactly the expected size) run on the host with at most min(n_images, 16) threads; the device
 *                 receives the inflated scanline stream, the palette and the geometry, never file bytes.
 *   unfilter      rowbytes = ceil(width x samples x depth / 8), bpp = max(1, samples x depth / 8).  For byte x of a row: a = the
 *                 reconstructed byte at x - bpp (0 when x < bpp), b = the reconstructed byte above (0 in row 0), c = the byte above
 *                 at x - bpp (0 when either is outside).  Predictors: None 0, Sub a, Up b, Average (a + b) >> 1 on the 9-bit sum,
 *                 Paeth with p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|: a if pa <= pb and pa <= pc, else b if
 *                 pb <= pc, else c.  The result is (filtered + predictor) & 255.
 *   pixels        depth 16 keeps the high byte; depth 1, 2, 4 gray scales by 255, 85, 17, packed samples MSB first; a palette index
 *                 looks up PLTE, an index at or past its length gives (0, 0, 0); alpha is dropped, not blended.  Colour types 0 and 4
 *                 come back as one channel (CV_8U), types 2, 3 and 6 as B, G, R interleaved (CV_8UC3); rows tight.
 *
 * sfmba_png_info: the chunk walk only (signature, CRCs, IHDR, PLTE, the IDAT list, IEND, the size gate), host only, no device needed;
 *   info [n_images].  A file whose chunks are in order reports SFMBA_IMAGE_OK here even when its zlib stream will prove corrupt in
 *   sfmba_png_decode.  channels is the number of OUTPUT channels (1 or 3).
 * sfmba_png_decode: as sfmba_jpeg_decode -- info [n_images] (the final status), out_ptr [n_images + 1], out [cap]; factor != 1 resizes
 *   before the pixels leave the device and equals factor = 1 followed by sfmba_resize_images byte for byte; a factor that gives an
 *   image a side outside 1..16384 is SFMBA_ERR_INVALID_ARG, judged from IHDR alone before anything is inflated.  A batch equals the
 *   concatenation of single-image calls.  SFMBA_ABI_VERSION stays 6: adding a symbol is backward compatible.
 */
/* The struct and the first function share their name, which a typedef cannot do in C: the struct is a TAG only, written
 * `struct sfmba_png_info` wherever it is meant. */
struct sfmba_png_info { int status; int width, height, channels; int bit_depth, colour_type, interlace; };
SFMBA_API int sfmba_png_info(int n_images, const int64_t* file_ptr /*[n_images+1], byte offsets*/, const unsigned char* bytes,
                struct sfmba_png_info* info /*[n_images]*/);
SFMBA_API int sfmba_png_decode(int device, int n_images, const int64_t* file_ptr /*[n_images+1], byte offsets*/,
                const unsigned char* bytes, float factor, struct sfmba_png_info* info /*[n_images]*/, int64_t* out_ptr /*[n_images+1]*/,
                unsigned char* out /*[cap]*/, int64_t cap, int64_t* total);

#ifdef __cplusplus
}
#endif
#endif /* SFMBA_H_ */
