/* mpcx -- C ABI of the MI355X-native batched MPC solve engine.
 *
 * This is the drop-in boundary for ONE path of libmpc++: what sits behind
 * IOptimizer<sizer>::run (reference include/mpc/IOptimizer.hpp:24-58), for a
 * *batch* of independent MPC instances that share one controller set-up:
 *   mpcx_lmpc_*   the linear back-end, LOptimizer::run + ProblemBuilder
 *                 (include/mpc/LMPC/LOptimizer.hpp:189-368, LMPC/ProblemBuilder.hpp);
 *   mpcx_nlmpc_*  the non-linear back-end, NLOptimizer::run with Mapping / Model /
 *                 Objective / Constraints (include/mpc/NLMPC/NLOptimizer.hpp:412-638);
 *   mpcx_discretize_batch  the c2d set-up helper (include/mpc/Utils.hpp:23-89);
 *   mpcx_dare_batch        Kalman and LQR gains for a batch of models (no reference counterpart).
 *   mpcx_target_map_batch  steady-state target maps for a batch of models (no reference counterpart).
 *
 * Conventions
 *   - plain C, opaque handle, no C++/torch types in any signature;
 *   - every matrix argument of a setter is a HOST pointer to column-major
 *     doubles (Eigen's default layout, reference include/mpc/Types.hpp:42);
 *   - every pointer inside mpcx_lmpc_batch is a DEVICE pointer (HBM), batch
 *     arrays are instance-major: x0[b*nx + j];
 *   - every call returns MPCX_OK (0) or a negative MPCX_E_* code; the per-instance
 *     outcome of a solve is reported in status[] / solver_status[] / is_feasible[]
 *     exactly like mpc::Result (Types.hpp:168-182).
 *   - horizon-slice semantics are the reference's: a slice is the half-open
 *     step range [start, end); {-1,-1} = whole horizon (Types.hpp:57-82,
 *     IMPC.hpp:244-283).  Replicate-along-horizon setters follow LMPC.hpp.
 */
#ifndef MPCX_H
#define MPCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCX_OK              0
#define MPCX_E_INVALID      -1   /* bad argument / dimension / slice            */
#define MPCX_E_UNSUPPORTED  -2   /* dimension outside what the kernels cover    */
#define MPCX_E_DEVICE       -3   /* HIP runtime error                           */
#define MPCX_E_NUMERIC      -4   /* set-up factorisation failed                 */
#define MPCX_E_STATE        -5   /* call order (e.g. solve before a model)      */

/* mpc::ResultStatus (Types.hpp:87-94) */
#define MPCX_STATUS_SUCCESS        0
#define MPCX_STATUS_MAX_ITERATION  1
#define MPCX_STATUS_INFEASIBLE     2
#define MPCX_STATUS_ERROR          3
#define MPCX_STATUS_UNKNOWN        4

/* solver_status: OSQP v0.6.3 status_val codes, which is what LOptimizer stores
 * in Result::solver_status (LOptimizer.hpp:342) */
#define MPCX_SOLVER_SOLVED               1
#define MPCX_SOLVER_SOLVED_INACCURATE    2
#define MPCX_SOLVER_MAX_ITER_REACHED    -2
#define MPCX_SOLVER_PRIMAL_INFEASIBLE   -3
#define MPCX_SOLVER_NON_CVX             -7
#define MPCX_SOLVER_UNSOLVED           -10

/* Dimensions: the run-time twin of MPCSize (reference include/mpc/Dim.hpp). */
typedef struct mpcx_dims {
    int nx, nu, ndu, ny, ph, ch;
} mpcx_dims;

/* POD mirror of mpc::LParameters (Types.hpp:99-114,146-161). */
typedef struct mpcx_lparams {
    int    maximum_iteration;   /* default 100 */
    double time_limit;          /* accepted, ignored (no wall clock inside a kernel) */
    int    enable_warm_start;   /* default 0 */
    double alpha;               /* 1.6  */
    double rho;                 /* 1e-6; used as the uniform ADMM step only when adaptive_rho == 0 */
    double eps_rel, eps_abs;    /* 1e-4 */
    double eps_prim_inf, eps_dual_inf;  /* 1e-3 */
    int    verbose;
    int    adaptive_rho;        /* 1: step sizes from the model's dual Hessian diagonal */
    int    polish;              /* 1: finish on the exact active-set solution, as OSQP's polish   */
} mpcx_lparams;

typedef struct mpcx_lmpc *mpcx_lmpc_t;

/* How a per-solve reference / exogenous-input array is laid out in HBM. */
#define MPCX_REF_SHARED        0  /* use the matrix given to the host setter (LMPC::setReferences) */
#define MPCX_REF_PER_INSTANCE  1  /* [B x n]      one vector per instance, constant along horizon  */
#define MPCX_REF_PER_STEP      2  /* [B x ph x n] full matrix per instance (column k = step k)     */

/* One batched LOptimizer::run.  All pointers are device pointers; optional
 * outputs may be NULL.  Replaces LOptimizer::run(x0,u0) (LOptimizer.hpp:189). */
typedef struct mpcx_lmpc_batch {
    int batch;
    const double *x0;              /* [B x nx]  measured state                                  */
    const double *u0;              /* [B x nu]  last applied input (lastU)                       */
    const double *yref;  int yref_mode;    /* output reference   (ny)  */
    const double *uref;  int uref_mode;    /* input reference    (nu)  */
    const double *duref; int duref_mode;   /* delta-u reference  (nu)  */
    const double *dmeas; int dmeas_mode;   /* exogenous inputs   (ndu) */
    /* Result<nu> as structure-of-arrays */
    double *cmd;                   /* [B x nu]  required: optimal first input, Result::cmd       */
    double *cost;                  /* [B]       0.5 z'Pz + q'z of the reference QP               */
    int32_t *status;               /* [B]       MPCX_STATUS_*                                    */
    int32_t *solver_status;        /* [B]       MPCX_SOLVER_*                                    */
    int32_t *is_feasible;          /* [B]                                                        */
    int32_t *iterations;           /* [B]       ADMM iterations spent                            */
    /* active set at the returned point, reference row numbering of A/l/u
     * (ProblemBuilder.hpp:814-822), one bit per row, [B x active_words] words */
    uint32_t *active_lower;
    uint32_t *active_upper;
    /* OptSequence (Types.hpp:184-198): row i = horizon step i, instance-major
     * [B x (ph+1) x n], row-major inside an instance */
    double *seq_state;
    double *seq_output;
    double *seq_input;
    /* extension, for work accounting: active-set (polish) rounds spent and size of the final
     * working set, [B] each */
    int32_t *polish_rounds;
    int32_t *active_count;
    /* warm start (inputs, may be NULL): the active_lower / active_upper words of the previous solve
     * of each instance.  The reference warm-starts OSQP with the previous primal/dual pair
     * (LOptimizer.hpp:268-281, LParameters::enable_warm_start); for the active-set iteration the
     * information that carries over is which rows were active: they are the first working set, and
     * an unchanged active set verifies in one round.  Results do not depend on it.               */
    const uint32_t *warm_active_lower;
    const uint32_t *warm_active_upper;
    int warm_shift;                /* 1: receding horizon -- the previous tick's row of step i+1 seeds step i */
} mpcx_lmpc_batch;

/* ---- lifetime (replaces LMPC::onSetup / new LOptimizer, LMPC.hpp:728-735) ---- */
int mpcx_lmpc_create(const mpcx_dims *dims, int device, mpcx_lmpc_t *out);
int mpcx_lmpc_destroy(mpcx_lmpc_t h);
void mpcx_lparams_default(mpcx_lparams *p);
const char *mpcx_last_error(void);

/* ---- controller set-up: names and semantics of LMPC.hpp ---------------------- */
/* LMPC::setStateSpaceModel (LMPC.hpp:493) */
int mpcx_lmpc_set_state_space_model(mpcx_lmpc_t h, const double *A, const double *B, const double *C);
/* LMPC::setDisturbances (LMPC.hpp:518) */
int mpcx_lmpc_set_disturbances(mpcx_lmpc_t h, const double *Bd, const double *Dd);
/* LMPC::setObjectiveWeights matrix form (LMPC.hpp:306) / vector+slice form (LMPC.hpp:436) */
int mpcx_lmpc_set_objective_weights(mpcx_lmpc_t h, const double *OW, const double *UW, const double *DUW);
int mpcx_lmpc_set_objective_weights_slice(mpcx_lmpc_t h, const double *ow, const double *uw, const double *duw,
                                          int start, int end);
/* LMPC::setStateBounds / setInputBounds / setOutputBounds (LMPC.hpp:111-292) */
int mpcx_lmpc_set_state_bounds(mpcx_lmpc_t h, const double *xmin, const double *xmax);
int mpcx_lmpc_set_state_bounds_slice(mpcx_lmpc_t h, const double *xmin, const double *xmax, int start, int end);
int mpcx_lmpc_set_input_bounds(mpcx_lmpc_t h, const double *umin, const double *umax);
int mpcx_lmpc_set_input_bounds_slice(mpcx_lmpc_t h, const double *umin, const double *umax, int start, int end);
int mpcx_lmpc_set_output_bounds(mpcx_lmpc_t h, const double *ymin, const double *ymax);
int mpcx_lmpc_set_output_bounds_slice(mpcx_lmpc_t h, const double *ymin, const double *ymax, int start, int end);
/* Bounds on the input rate, dumin <= u_k - u_{k-1} <= dumax.  The reference's QP carries these rows -- ProblemBuilder.hpp:768-793
 * builds ph*nu inequality rows on the delta-u variables, free (+-inf) for steps i <= ch and pinned to 0 behind the control
 * horizon -- but the reference has no setter for them: this one goes beyond its surface and stays inside its QP.
 * [nu x ph] column-major; column i bounds delta_i = v_{i+1} - v_i with v_0 = lastU (DeltaUWeight's indexing, no column shift).
 * Columns i > ch are stored and not read (those moves stay pinned).  Default +-inf.  The slice form takes a prediction-horizon
 * slice like the delta-u weight's.  MPCX_E_INVALID: null pointer, NaN, or dumin > dumax in a column <= ch. */
int mpcx_lmpc_set_input_rate_bounds(mpcx_lmpc_t h, const double *dumin, const double *dumax);
int mpcx_lmpc_set_input_rate_bounds_slice(mpcx_lmpc_t h, const double *dumin, const double *dumax, int start, int end);
/* Soft constraints: a weight rho in (0, +inf] for each state row, output row and the scalar row; +inf (the default) keeps the row hard.  A
 * finite weight replaces the row lo <= g <= hi by the term 0.5 rho dist^2(g, [lo, hi]) in the cost -- one free slack per row with cost
 * 0.5 rho s^2.  The reference's LMPC has no counterpart (its NLMPC has one slack for all rows, NLOptimizer.hpp:182-186).  Input bounds and
 * input-rate bounds stay hard.  xw[nx], yw[ny], sw[1]; a null pointer leaves that kind of row as it is.  The first form sets the whole
 * horizon, steps 0 .. ph; the slice form has the slice semantics and the column shift of mpcx_lmpc_set_state_bounds_slice, so that a weight
 * softens exactly the rows the same call of the bounds setter bounds (sw as mpcx_lmpc_set_scalar_constraint_slice).  A weight where no
 * bound is finite is stored and has no effect.  A soft row never makes an instance infeasible, strict mode included (a soft step-0 row, which
 * sees no decision variable, is then a pure cost term); `cost` includes the penalty; the active bit of a soft row is set when its multiplier is
 * non-zero, i.e. when the row is violated or on its bound with a pull; row numbering, m_ref and active_words do not change.
 * MPCX_E_INVALID: NaN, zero or a negative weight; a slice out of bounds. */
int mpcx_lmpc_set_soft_constraint_weights(mpcx_lmpc_t h, const double *xw, const double *yw, const double *sw);
int mpcx_lmpc_set_soft_constraint_weights_slice(mpcx_lmpc_t h, const double *xw, const double *yw, const double *sw, int start, int end);
/* Terminal cost: the term 0.5 (x_ph - x_T)' P (x_ph - x_T) on the last predicted state, with
 *     x_T = xT + Tr yref(., ph - 1) + Td dmeas(., ph - 1),   Tx = [Tr | Td]  [nx x (ny + ndu)] column-major.
 * P [nx x nx] column-major, symmetric positive semidefinite -- with the cost-to-go of the unconstrained problem (mpcx_dare_batch, control form)
 * a short horizon behaves like an infinite one.  xT [nx] is a constant target; the columns of Tx are the first ny + ndu columns of map_x of
 * mpcx_target_map_batch, so that the target follows the instance's own output reference (shared, per-instance or per-step: the column step ph
 * reads) and its own exogenous input -- the disturbance estimate in an offset-free loop.  A null xT or Tx means zeros; a null P removes the term.
 * x_ph is the state reached with the blocked inputs.  `cost` stays 0.5 z' P z + q' z of the QP: the constant 0.5 x_T' P x_T is dropped, as
 * 0.5 r' W r of the output term is.  Row numbering, m_ref and active_words do not change.  The reference's LMPC has no counterpart
 * (DESIGN.md 3.3).  MPCX_E_INVALID, nothing stored: a NaN or infinite entry; |P - P'|_max > 1e-10 |P|_max (below that the symmetrised
 * matrix is stored); a smallest eigenvalue below -1e-10 |P|_max. */
int mpcx_lmpc_set_terminal_cost(mpcx_lmpc_t h, const double *P, const double *xT, const double *Tx);
/* LMPC::setScalarConstraint slice form (LMPC.hpp:355) and index form (LMPC.hpp:409) */
int mpcx_lmpc_set_scalar_constraint_slice(mpcx_lmpc_t h, double smin, double smax, const double *X, const double *U,
                                          int start, int end);
int mpcx_lmpc_set_scalar_constraint_index(mpcx_lmpc_t h, int index, double smin, double smax,
                                          const double *X, const double *U);
/* Linear constraints: nc rows with coefficients shared by all steps and bounds per step,
 *     lo[c, i] <= Fx[c, :] x_i + Fu[c, :] v_i <= hi[c, i],   i = 0 .. ph,   v_i = x_u(i) = u_{i-1}, v_0 = lastU
 * -- the scalar row's convention for nc rows: half-plane sets on the state, limits on combinations of actuators, rows that couple state and input,
 * and with bounds at the last step only a polytopic terminal set.  The reference's LMPC has no counterpart.  Fx [nc x nx],
 * Fu [nc x nu] column-major.  An infinite side is absent, a row with both sides infinite does not exist, lo == hi is an equality.  Default: no rows.
 * The first form sets the whole horizon, lo and hi [nc x (ph + 1)] column-major, column i = step i; nc = 0 removes the rows (the other arguments
 * are then not read).  The slice form takes lo[nc], hi[nc] and has the slice semantics and the column shift of
 * mpcx_lmpc_set_scalar_constraint_slice: slice index i bounds step i + 1, index 0 also step 0, (-1, -1) every step; the slice (ph - 1, ph) is the
 * terminal set.  The coefficients it brings replace the stored ones at every step.  A step-0 row sees no decision variable: a hard one is a
 * feasibility condition on (x0, lastU).
 * Row numbering: the rows are appended behind the reference's own, step i row c at m_ref(reference) + i nc + c; m_ref and active_words grow by
 * (ph + 1) nc for a controller that has such a row with a finite bound, and for no other.
 * nc <= MPCX_MAX_LINEAR_ROWS.  The cap is the LDS the coefficient block takes in lmpc_assemble_generic: nc (nx + nu) doubles in every
 * wavefront's slice, next to the roll-out's arrays -- 16 KB per wavefront at the largest model the kernels take (nx = nu = 64), a tenth of a
 * compute unit's LDS, and 2 KB at the quadrotor's nx = 12, nu = 4.
 * MPCX_E_INVALID, nothing stored: a null pointer with nc > 0; a NaN entry; an infinite coefficient; lo > hi; nc < 0 or above the cap; a slice
 * out of bounds or with nc = 0; a slice whose nc differs from the stored one while a step outside the slice holds a finite bound. */
#define MPCX_MAX_LINEAR_ROWS 16
int mpcx_lmpc_set_linear_constraints(mpcx_lmpc_t h, int nc, const double *Fx, const double *Fu, const double *lo, const double *hi);
int mpcx_lmpc_set_linear_constraints_slice(mpcx_lmpc_t h, int nc, const double *Fx, const double *Fu, const double *lo, const double *hi,
                                           int start, int end);
/* Soft weights of the linear rows, w[nc] with the stored nc, under the rules of mpcx_lmpc_set_soft_constraint_weights: rho in (0, +inf], +inf (the
 * default) keeps the row hard, a finite weight replaces the row by 0.5 rho dist^2 in the cost.  The first form sets steps 0 .. ph, the slice
 * form has the slice semantics of mpcx_lmpc_set_linear_constraints_slice.  The weights stay with the rows while calls of the bounds setters keep
 * nc; a call that changes nc makes every row hard again.  MPCX_E_INVALID: null pointer, NaN, zero or a negative weight; a slice out of bounds. */
int mpcx_lmpc_set_linear_constraint_weights(mpcx_lmpc_t h, const double *w);
int mpcx_lmpc_set_linear_constraint_weights_slice(mpcx_lmpc_t h, const double *w, int start, int end);
/* LMPC::setReferences matrix form (LMPC.hpp:596) / vector+slice form (LMPC.hpp:616) */
int mpcx_lmpc_set_references(mpcx_lmpc_t h, const double *yref, const double *uref, const double *duref);
int mpcx_lmpc_set_references_slice(mpcx_lmpc_t h, const double *yref, const double *uref, const double *duref,
                                   int start, int end);
/* LMPC::setExogenousInputs matrix form (LMPC.hpp:534) / vector+slice form (LMPC.hpp:550) */
int mpcx_lmpc_set_exogenous_inputs(mpcx_lmpc_t h, const double *dmeas);
int mpcx_lmpc_set_exogenous_inputs_slice(mpcx_lmpc_t h, const double *dmeas, int start, int end);
/* LMPC::setOptimizerParameters -> LOptimizer::setParameters (LMPC.hpp:79, LOptimizer.hpp:100) */
int mpcx_lmpc_set_optimizer_parameters(mpcx_lmpc_t h, const mpcx_lparams *p);

/* Extension (no reference counterpart).  With the reference an infeasible QP is never reported
 * INFEASIBLE: libmpc++ hands OSQP true infinities, OSQP v0.6.3's certificate test then evaluates
 * inf*0 = NaN and never fires, the solve runs out of iterations and LOptimizer returns the last
 * ADMM iterate flagged MAX_ITERATION / is_feasible = true (LOptimizer.hpp:344).  Default (0):
 * same flags, cmd = the optimum of the QP without the rows that (x0, lastU) alone violate, or the
 * last ADMM iterate when the infeasibility involves the inputs.  1: status INFEASIBLE, cmd = NaN. */
int mpcx_lmpc_set_strict_infeasibility(mpcx_lmpc_t h, int on);

/* ---- the hot path --------------------------------------------------------------- */
/* Condense the controller into device-resident matrices.  Called implicitly by
 * the first solve after any setter; exposed so that set-up cost can be paid
 * (and timed) up front. */
int mpcx_lmpc_setup(mpcx_lmpc_t h);
/* Batched LOptimizer::run on `stream` (a hipStream_t, NULL = default stream).
 * Asynchronous with respect to the host; outputs are valid once the stream
 * has been synchronised.
 * Concurrency: a handle owns ONE per-instance workspace and ONE set of dispatch queues.  Launches of the
 * same handle on the same stream are ordered and safe; two launches of the same handle in flight on
 * DIFFERENT streams race on them (instances could be dropped or solved twice).  Overlap batches by giving
 * each stream its own handle (set-up cost is per handle and paid once), as bench.py's pipelined leg does.
 * maximum_iteration: the main iteration here is OSQP's polish step repeated until the KKT conditions verify
 * (DESIGN.md 4.3); it needs no ADMM iterations, so LParameters::maximum_iteration only bounds the ADMM
 * fallback that takes over when the polish does not verify (or when polish = 0).  `iterations[]` reports
 * the ADMM iterations actually spent (0 on the polish path), `polish_rounds[]` the active-set rounds.  A QP the
 * reference would leave MAX_ITER_REACHED and un-polished comes back here as the exact optimum with SUCCESS. */
int mpcx_lmpc_solve_batch(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream);
/* Same launch, timed with HIP events recorded on `stream` around `repeats`
 * back-to-back launches; returns the mean kernel time in milliseconds. */
int mpcx_lmpc_time_solve_batch(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, int repeats, float *ms_mean);

/* Sensitivities of a solved batch: the slope of the solution on each instance's active set.  On the working set a
 * solve ended with, the decision vector is affine in (x0, lastU, yref); one launch evaluates the transpose of that map per instance.
 *   MPCX_SENS_JACOBIAN  the local feedback law cmd ~ cmd* + d_x0 (x - x0) + d_u0 (lastU - u0) + d_yref (yref - yref0):
 *                       d_x0 [B x nu x nx], d_u0 [B x nu x nu], d_yref [B x nu x ny], row-major, rows = components of cmd
 *   MPCX_SENS_VJP       one cotangent per instance: seed_cmd [B x nu] on cmd and / or seed_input [B x (ph + 1) x nu] on the input sequence
 *                       as the solve writes it (row i = the input of step min(i + 1, ph); row 0 is cmd); d_x0 [B x nx], d_u0 [B x nu],
 *                       d_yref [B x ny] are the gradients of sum(seed * output)
 * active_lower / active_upper are the words a solve of this handle wrote (required); which side a row is active on does not enter.  All
 * pointers are device pointers; every output may be NULL.  status (optional): an instance whose status is not MPCX_STATUS_SUCCESS gets
 * flag 1.  flags (optional): 0 fine; 1 not solved; 2 the working set is linearly dependent (the derivative does not exist there);
 * 3 the working set has more rows than the kernel's LDS plan holds.  The outputs of an instance with a non-zero flag are NaN.
 * d_x0 and d_u0 hold for every reference mode of the solve that produced the active sets: the linear part of the maps does not depend on
 * references or exogenous inputs.  d_yref is the derivative with respect to a shift of the output reference common to all steps: the
 * exact Jacobian for MPCX_REF_PER_INSTANCE, a directional derivative for the other modes.
 * Asynchronous on `stream`, like the solve; allocates nothing.  Banks (mpcx_lmpc_hetero_*): mpcx_lmpc_hetero_sensitivity_batch. */
#define MPCX_SENS_JACOBIAN 0
#define MPCX_SENS_VJP      1
typedef struct mpcx_lmpc_sens {
    int batch;
    const uint32_t *active_lower, *active_upper;  /* [B x active_words], device, as a solve wrote them */
    const int32_t *status;       /* optional [B] */
    int mode;                    /* MPCX_SENS_JACOBIAN | MPCX_SENS_VJP */
    const double *seed_cmd;      /* VJP: [B x nu], may be NULL */
    const double *seed_input;    /* VJP: [B x (ph+1) x nu], may be NULL (not both) */
    double *d_x0, *d_u0, *d_yref;
    int32_t *flags;              /* optional [B] */
} mpcx_lmpc_sens;
int mpcx_lmpc_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_sens *s, void *stream);
int mpcx_lmpc_sens_size(void);   /* sizeof(mpcx_lmpc_sens), for bindings that mirror the struct */
/* Host-array form for callers without a device allocator (mpc::LMPC<>::sensitivities): the Jacobians of the batch the last
 * mpcx_lmpc_solve_host of this handle solved, on the active sets and status that call left on the device; d_x0 [B x nu x nx],
 * d_u0 [B x nu x nu], d_yref [B x nu x ny] row-major and flags [B] on the host, each may be NULL.  Synchronous.  MPCX_E_STATE without
 * such a solve, or after a change of the controller. */
int mpcx_lmpc_sensitivity_host(mpcx_lmpc_t h, double *d_x0, double *d_u0, double *d_yref, int32_t *flags);

/* Parameter sensitivities of a solved batch: the gradient of sum(seed * output) -- seeds on cmd and / or on the input sequence,
 * exactly as MPCX_SENS_VJP takes them, one per instance -- with respect to the three weight matrices of mpcx_lmpc_set_objective_weights and to
 * every bound of the QP, on the active set each instance was solved on.  One launch after the solve; a second small one adds up the batch.
 *   solved      the batch descriptor a solve of this handle filled, unchanged since: x0, u0, the references in their modes, seq_output,
 *               seq_input, active_lower, active_upper (all required) and status (optional: an unsolved instance gets flag 1)
 *   reduce      0: an output set per instance, d_oweight [B x (ny x ph)], d_uweight, d_duweight [B x (nu x ph)], each matrix column-major as
 *               the setter takes it (column = user step), d_lower, d_upper [B x m_ref]; 1: one set, the sum over the instances whose flag is 0,
 *               added in a fixed order without floating-point atomics (two launches give the same bits), and n_used [1] = how many those were.
 *               reduce = 1 takes its partial sums from a buffer of the handle: mpcx_lmpc_param_sens_reserve(h, batch) once, outside any
 *               capture, for the largest batch (MPCX_E_STATE otherwise); the launch itself allocates nothing
 *   d_lower / d_upper   one entry per row the active words name (mpcx_lmpc_info.m_ref, the linear rows included), in that numbering: the
 *               multiplier of the adjoint system on the side whose bit is set (the upper one where both are), zero for every other row and
 *               for rows without decision variables (the step-0 box rows).  A condensed variable bounded by several reference rows (move
 *               blocking) files the whole value under the lowest-numbered row whose bit is set
 * flags: the codes of mpcx_lmpc_sens -- 0 fine, 1 not solved, 2 dependent working set, 3 beyond the LDS plan; with reduce = 0 the outputs of a flagged
 * instance are NaN.  All pointers are device pointers, every output may be NULL.  MPCX_E_STATE when the controller changed, or was set up
 * again, since this handle's last mpcx_lmpc_solve_batch: the batch must be the one that call solved.  Not differentiated here: the model (mpcx_lmpc_model_sensitivity_batch has it), the terminal weight, soft weights, the coefficients of scalar and linear rows.
 * Asynchronous on `stream`; neither form allocates or copies at launch: the kernel's operand Cq is uploaded by the set-up, the partial sums of
 * reduce = 1 by mpcx_lmpc_param_sens_reserve.  With reduce = 1 and both d_lower and d_upper NULL the bound rows are not computed at all.
 * Banks (mpcx_lmpc_hetero_*): mpcx_lmpc_hetero_gradient_batch, per instance and summed per controller. */
typedef struct mpcx_lmpc_param_sens {
    const mpcx_lmpc_batch *solved;
    const double *seed_cmd, *seed_input;          /* [B x nu], [B x (ph+1) x nu]; at least one */
    int reduce;
    double *d_oweight, *d_uweight, *d_duweight;
    double *d_lower, *d_upper;
    int32_t *flags;                               /* optional [B] */
    int32_t *n_used;                              /* optional [1], reduce = 1 only */
} mpcx_lmpc_param_sens;
int mpcx_lmpc_param_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_param_sens *s, void *stream);
int mpcx_lmpc_param_sens_size(void);   /* sizeof(mpcx_lmpc_param_sens) */
int mpcx_lmpc_param_sens_reserve(mpcx_lmpc_t h, int batch);      /* the partial sums of reduce = 1 for batches up to `batch` (grow-only) */
/* Host-array form over the batch the last mpcx_lmpc_solve_host of this handle solved with its sequences asked for (mpc::LMPC<>::
 * parameterSensitivities): seeds and outputs on the host, laid out as above; synchronous.  MPCX_E_STATE without such a solve. */
int mpcx_lmpc_param_sensitivity_host(mpcx_lmpc_t h, const double *seed_cmd, const double *seed_input, int reduce,
                                     double *d_oweight, double *d_uweight, double *d_duweight, double *d_lower, double *d_upper,
                                     int32_t *flags, int32_t *n_used);

/* Model sensitivities of a solved batch: the gradient of sum(seed * output) -- seeds as mpcx_lmpc_param_sens takes them -- with
 * respect to every entry of the model's matrices A [nx x nx], B [nx x nu], C [ny x nx], Bd [nx x ndu] and Dd [ny x ndu], on the active set each
 * instance was solved on.  One launch after the solve; a second small one adds up the batch.
 *   solved      as for mpcx_lmpc_param_sens, and seq_state as well; the exogenous inputs in their mode
 *   reduce      0: a set per instance, [B x ..], each matrix column-major as mpcx_lmpc_set_state_space_model / _set_disturbances take it;
 *               1: one set, the sum over the instances whose flag is 0 in a fixed order (two launches give the same bits), n_used [1] = how
 *               many those were.  reduce = 1 needs mpcx_lmpc_model_sens_reserve(h, batch) once, outside any capture (MPCX_E_STATE otherwise)
 * flags as in mpcx_lmpc_param_sens; with reduce = 0 the outputs of a flagged instance are NaN.  All pointers are device pointers, every output
 * may be NULL; d_Bd / d_Dd are ignored without exogenous inputs.  MPCX_E_STATE under the rules of mpcx_lmpc_param_sensitivity_batch.
 * The multipliers of the optimum are recomputed from its own sequences, so every reference mode of the solved batch is served.
 * Not differentiated: soft weights, the terminal weight, its target and target map, the coefficients of scalar and linear rows; step 0.
 * Asynchronous on `stream`; the launch allocates nothing: the kernel's operand Xq is built and uploaded by mpcx_lmpc_model_sens_reserve or by
 * the first launch outside a capture after a set-up (a launch under capture without either: MPCX_E_STATE).  Banks (mpcx_lmpc_hetero_*): mpcx_lmpc_hetero_gradient_batch. */
typedef struct mpcx_lmpc_model_sens {
    const mpcx_lmpc_batch *solved;
    const double *seed_cmd, *seed_input;          /* [B x nu], [B x (ph+1) x nu]; at least one */
    int reduce;
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;
    int32_t *flags;                               /* optional [B] */
    int32_t *n_used;                              /* optional [1], reduce = 1 only */
} mpcx_lmpc_model_sens;
int mpcx_lmpc_model_sensitivity_batch(mpcx_lmpc_t h, const mpcx_lmpc_model_sens *s, void *stream);
int mpcx_lmpc_model_sens_size(void);   /* sizeof(mpcx_lmpc_model_sens) */
int mpcx_lmpc_model_sens_reserve(mpcx_lmpc_t h, int batch);      /* Xq of the current set-up, and the partial sums of reduce = 1 for batches up to `batch` (grow-only; 0: Xq alone) */
/* Host-array form over the batch the last mpcx_lmpc_solve_host of this handle solved with its sequences asked for (mpc::LMPC<>::
 * modelSensitivities): seeds and outputs on the host, laid out as above; synchronous.  MPCX_E_STATE without such a solve. */
int mpcx_lmpc_model_sensitivity_host(mpcx_lmpc_t h, const double *seed_cmd, const double *seed_input, int reduce,
                                     double *d_A, double *d_B, double *d_C, double *d_Bd, double *d_Dd, int32_t *flags, int32_t *n_used);

/* One step as a HIP graph.  A control loop solves the same-sized batch from the same buffers every tick: the launches of
 * one mpcx_lmpc_solve_batch (dispatch-queue reset, assemble, solve, fallback) are captured once for a batch descriptor and
 * replayed with a single hipGraphLaunch.  The descriptor's pointers are baked into the graph; what they point to may change
 * between launches (new x0, u0, references), the controller's set-up may not (create a new graph after a setter).
 * `stream` of create: any non-default stream (used for one untimed warm-up solve and for the capture).  A handle still
 * has one workspace: one launch of it in flight at a time, graph or not.                                          */
typedef struct mpcx_lmpc_graph *mpcx_lmpc_graph_t;
int mpcx_lmpc_graph_create(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, mpcx_lmpc_graph_t *out);
int mpcx_lmpc_graph_launch(mpcx_lmpc_graph_t g, void *stream);
int mpcx_lmpc_graph_destroy(mpcx_lmpc_graph_t g);

/* The closed loop on the device (no reference counterpart: there the loop is the caller's `for`, examples/quadrotor_ex.cpp).  `ticks`
 * receding-horizon steps of `batch` instances of one controller -- closed-loop Monte-Carlo runs, or a fleet in lock step: tick k is the batched
 * solve of mpcx_lmpc_solve_batch (same kernels, same choice of them) on the loop's own current state and last input, followed by one kernel that
 * steps the plant, x <- A_p x + B_p cmd + Bd_p d_k + w_k (d_k: step 0 of the tick's exogenous input, what the controller's own prediction uses
 * for its first transition), makes cmd the next tick's last input (as it is, unclipped), logs the tick and prepares the next one.  Both are
 * captured in a HIP graph; between ticks the host only enqueues graph launches.
 * References: the modes of mpcx_lmpc_batch mean the same thing at every tick; MPCX_REF_PREVIEW is an array [B x (ticks + ph) x n] of which tick k
 * sees rows k .. k + ph - 1 as its MPCX_REF_PER_STEP matrix (and the plant row k of dmeas).
 * Trajectories are tick-major: traj_x [(ticks + 1) x B x nx] (row 0 = x0), traj_u [ticks x B x nu], the optional ones [ticks x B].
 * A loop uses its handle's one workspace: the concurrency rule of mpcx_lmpc_solve_batch holds unchanged, a run counts as a launch in flight until
 * the stream has been synchronised.  A setter on the controller invalidates the loop (mpcx_lmpc_loop_run returns MPCX_E_STATE): create a new one.
 * The plant: the controller's own model, one other plant for the whole batch (plant_A / _B / _Bd), or a plant per instance (plant_batch, a
 * Monte-Carlo run over B plants); the last goes through a second advance kernel whose lanes are (instance, state row) pairs and which agrees bit
 * for bit with the first on equal plants.  plant_batch is a device array read at the head of every run, like x0 / u0: refill it in place. */
#define MPCX_REF_PREVIEW       3  /* loops only: [B x (ticks + ph) x n], a window of ph rows per tick */
typedef struct mpcx_lmpc_loop_desc {
    int batch, ticks;
    const double *plant_A, *plant_B, *plant_Bd;   /* HOST, column-major [nx x nx], [nx x nu], [nx x ndu]; NULL = the controller's own */
    const double *x0, *u0;                        /* device, [B x nx], [B x nu]: initial state and last input, read again by every run */
    const double *yref;  int yref_mode;           /* device, as in mpcx_lmpc_batch, or MPCX_REF_PREVIEW */
    const double *uref;  int uref_mode;
    const double *duref; int duref_mode;
    const double *dmeas; int dmeas_mode;
    const double *noise;                          /* device, [ticks x B x nx] additive process disturbance w_k, or NULL */
    int carry_working_set;                        /* 1: tick k's active sets warm-start tick k + 1 (warm_shift = 1); tick 0 is cold */
    double *traj_x, *traj_u;                      /* device, required */
    double *traj_cost;                            /* device, optional from here on */
    int32_t *traj_status, *traj_solver_status, *traj_iterations, *traj_polish_rounds, *traj_active_count;
    const double *plant_batch;                    /* device, [B x nx (nx + nu + ndu)]: A_b | B_b | Bd_b per instance, each column-major, read again by
                                                     every run; NULL = one plant for the batch.  Excludes plant_A / plant_B / plant_Bd */
} mpcx_lmpc_loop_desc;
typedef struct mpcx_lmpc_loop *mpcx_lmpc_loop_t;
/* `stream`: any non-default stream (warm-up solves and the capture, as for mpcx_lmpc_graph_create).  The descriptor's device pointers are baked
 * into the graph; what they point to may change between runs. */
int mpcx_lmpc_loop_create(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, void *stream, mpcx_lmpc_loop_t *out);
/* asynchronous: resets the tick counter, reads x0 / u0 again, enqueues the ticks; the trajectories are valid once `stream` has been synchronised */
int mpcx_lmpc_loop_run(mpcx_lmpc_loop_t l, void *stream);
int mpcx_lmpc_loop_destroy(mpcx_lmpc_loop_t l);
int mpcx_lmpc_loop_desc_size(void);               /* sizeof(mpcx_lmpc_loop_desc), for bindings that mirror the struct */

/* The backward pass of that loop (no reference counterpart: the reference has neither the loop nor a derivative).  Given cotangents
 * on the logged trajectories, one run returns the gradient of sum(seed_x * traj_x) + sum(seed_u * traj_u) of the loop's last completed run with
 * respect to the initial state and last input, the output reference, the process noise, the plant, the controller's weights and its model.
 * The adjoint recursion runs tick ticks - 1 down to 0 with lambda_ticks = seed_x[ticks], mu_ticks = 0 and the instance's plant A_p, B_p, Bd_p:
 *     c_k = seed_u[k] + B_p' lambda_{k+1} + mu_{k+1}               the cotangent on cmd_k (which is also lastU of tick k + 1)
 *     (gx, gu, gy, gtheta) = the vector-Jacobian products of tick k's solve seeded with c_k     (mpcx_lmpc_sensitivity_batch in MPCX_SENS_VJP mode,
 *                                                                   mpcx_lmpc_param_sensitivity_batch, mpcx_lmpc_model_sensitivity_batch)
 *     lambda_k = seed_x[k] + A_p' lambda_{k+1} + gx,  mu_k = gu
 *     d_yref += gy,  d_theta += gtheta,  d_noise[k] = lambda_{k+1},  d_plant += lambda_{k+1} [x_k; cmd_k; d_k]'
 * and d_x0 = lambda_0, d_u0 = mu_0.  The solve of tick k is computed again, cold, from traj_x[k], traj_u[k - 1] (the loop's u0 at tick 0) and the
 * tick's references in the loop's modes (MPCX_REF_PREVIEW: the window at row k): the QP is strictly convex, so this is the point the forward run
 * reached, with or without carried working sets.  Nothing is taped beyond the two trajectories; memory does not grow with ticks.  A backward tick
 * (re-solve, the VJP launches, one adjoint kernel) is captured once as a linear chain; a run is a begin kernel, `ticks` replays and a finish step,
 * with no host work in between and nothing allocated.
 *   reduce      d_plant, the weights and the model: 0 a set per instance [B x ..]; 1 one set, the sum over the instances whose flag is 0, added in a
 *               fixed order without floating-point atomics (two runs give the same bits), and n_used [1] = how many those were.  d_x0, d_u0,
 *               d_yref and d_noise are per instance always
 *   d_yref      what mpcx_lmpc_sens.d_yref means: a shift common to all steps, and here to all ticks; exact for MPCX_REF_PER_INSTANCE
 *   d_plant     [B x nx (nx + nu + ndu)] (reduce = 1: one row): A_p | B_p | Bd_p, each column-major -- plant_batch's layout -- whichever plant the
 *               loop has; the controller's model enters it only as the plant, its part in the solves is d_A .. d_Dd
 *   flags       [B]: 0, or the OR over the ticks of the codes of mpcx_lmpc_sens.  An instance with a flag has NaN in every per-instance output
 *               and enters no sum
 * Every output may be NULL, and what nobody asks for is not computed: no model launch without one of d_A .. d_Dd, no sequences in the re-solve
 * without weights or model.  MPCX_E_INVALID, ahead of any look at the loop's state, for a null descriptor, both seeds NULL, and a loop that is
 * observed, offset-free, with targets, or a bank's: those are follow-ups.  MPCX_E_STATE under the loop's own invalidation rule (a setter since
 * its creation).  `stream` of create: any non-default stream (one plain backward tick and the capture).  _run comes after a completed
 * mpcx_lmpc_loop_run of the loop, on the same stream or synchronised with it; it uses the handle's one workspace and overwrites the loop's private
 * solve buffers, not its trajectories: the concurrency rule of mpcx_lmpc_loop_run holds.  The seeds and the trajectories are read again by every
 * run: refill them in place.  Destroy the gradient before its loop.
 * Not differentiated: bounds, soft weights, the terminal weight, the coefficients of scalar and linear rows, dmeas, uref.  Banks and loops with an
 * estimator have no backward pass yet. */
typedef struct mpcx_lmpc_loop_grad_desc {
    const double *seed_x;        /* device [(ticks+1) x B x nx] or NULL */
    const double *seed_u;        /* device [ticks x B x nu] or NULL (not both NULL) */
    int reduce;                  /* plant / weights / model: 0 per instance [B x ..], 1 summed over the instances with flag 0 */
    double *d_x0, *d_u0, *d_yref;                     /* [B x nx], [B x nu], [B x ny] */
    double *d_noise;                                  /* [ticks x B x nx] */
    double *d_plant;                                  /* plant_batch's layout per instance: A | B | Bd, each column-major */
    double *d_oweight, *d_uweight, *d_duweight;       /* layouts of mpcx_lmpc_param_sens */
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;            /* layouts of mpcx_lmpc_model_sens */
    int32_t *flags;                                   /* [B]: 0, or the OR over ticks of the codes of mpcx_lmpc_sens */
    int32_t *n_used;                                  /* [1], reduce = 1 */
} mpcx_lmpc_loop_grad_desc;
typedef struct mpcx_lmpc_loop_grad *mpcx_lmpc_loop_grad_t;
int mpcx_lmpc_loop_grad_create(mpcx_lmpc_loop_t l, const mpcx_lmpc_loop_grad_desc *g, void *stream, mpcx_lmpc_loop_grad_t *out);
int mpcx_lmpc_loop_grad_run(mpcx_lmpc_loop_grad_t g, void *stream);   /* after a completed mpcx_lmpc_loop_run of l, same stream or synchronised */
int mpcx_lmpc_loop_grad_destroy(mpcx_lmpc_loop_grad_t g);
int mpcx_lmpc_loop_grad_desc_size(void);          /* sizeof(mpcx_lmpc_loop_grad_desc), for bindings that mirror the struct */

/* Output feedback for that loop (no reference counterpart: the reference has neither the loop nor an observer; its examples hand optimize() the
 * plant's state).  An observed loop carries the true state x and an estimate xhat per instance; the solve of tick k reads xhat_k and u_{k-1}, and
 * the advance kernel computes, everything from tick-k data (predictor form, so every reference and dmeas mode works unchanged):
 *     y_k     = C x_k + Dd d_k + v_k            the measurement, v_k the optional sensor noise
 *     e_k     = y_k - (C xhat_k + Dd d_k)
 *     x_k+1   = A_p x_k + B_p cmd_k + Bd_p d_k + w_k          as in an unobserved loop
 *     xhat_k+1 = A xhat_k + B cmd_k + Bd d_k + L e_k
 * with A, B, Bd, C, Dd the controller's own model and the plant whatever the loop descriptor says.  Every row is summed from 0 with fused
 * multiply-adds by ascending column -- y over C, then Dd, then + v_k; xhat over A, B, Bd, then L -- so that e_k is an exact 0 where xhat_k equals
 * x_k bitwise and there is no sensor noise, and an observed loop on the controller's own plant without noise reproduces the unobserved loop.
 * xhat_0 is xhat0, or x0.  The loop is an mpcx_lmpc_loop_t: _run, _destroy, _debug_replay and _debug_tick serve it, invalidation is unchanged.
 * gain is copied at creation; gain_batch, xhat0 and meas_noise are device arrays read by every run: refill them in place. */
typedef struct mpcx_lmpc_observer_desc {
    const double *gain;                           /* HOST, column-major [nx x ny]: one gain for the batch, or NULL */
    const double *gain_batch;                     /* device, [B x nx*ny], per instance, column-major, read at the head of every run; excludes gain */
    const double *xhat0;                          /* device [B x nx] or NULL (= x0), read again by every run */
    const double *meas_noise;                     /* device [ticks x B x ny] or NULL */
    double *traj_xhat;                            /* device [(ticks+1) x B x nx], optional */
    double *traj_y;                               /* device [ticks x B x ny], optional */
} mpcx_lmpc_observer_desc;
/* mpcx_lmpc_loop_create with an observer (no reference counterpart).  MPCX_E_INVALID, ahead of any look at the handle's state, for a null observer
 * and for neither or both of gain / gain_batch. */
int mpcx_lmpc_loop_create_observed(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_observer_desc *o, void *stream, mpcx_lmpc_loop_t *out);
int mpcx_lmpc_observer_desc_size(void);           /* sizeof(mpcx_lmpc_observer_desc), for bindings that mirror the struct */
/* Offset-free tracking for that loop (no reference counterpart): an observed loop whose estimator carries [xhat; dhat], the integrating disturbance
 * model of the controller's own Bd / Dd (mpcx_lmpc_set_disturbances).  When the plant is not the model, or a constant load acts on it that nobody
 * measures, a state observer alone settles on a biased estimate and every instance beside its reference; here the bias is estimated and handed to
 * the solve.  The solve of tick k reads xhat_k, u_{k-1} and dhat_k -- the loop's own [B x ndu] buffer as its MPCX_REF_PER_INSTANCE exogenous
 * input, hence constant along the horizon -- and the loop descriptor's dmeas, in every mode it has, is no longer what the controller is told: it
 * is the TRUE disturbance d_k (step 0 of the tick's array) that acts on the plant and on the measurement, unseen by the controller.  dmeas = NULL
 * in MPCX_REF_SHARED mode means the controller's own exogenous input (a bank: each controller's own): zeros unless it was set.  Per tick,
 * everything from tick-k data:
 *     y_k      = C x_k + Dd d_k + v_k
 *     e_k      = y_k - (C xhat_k + Dd dhat_k)
 *     x_k+1    = A_p x_k + B_p cmd_k + Bd_p d_k + w_k
 *     xhat_k+1 = A xhat_k + B cmd_k + Bd dhat_k + Lx e_k
 *     dhat_k+1 = dhat_k + Ld e_k
 * with the gain [(nx + ndu) x ny] = [Lx; Ld].  Every row is summed from 0 with fused multiply-adds by ascending column -- y over C, Dd (operand
 * d_k), then + v_k; yhat over C, Dd (operand dhat_k); xhat over A, B, Bd (operand dhat_k), Lx, nothing added at the store; the correction of dhat
 * over Ld from 0, added to dhat_k once -- so that with Ld = 0, dhat_0 = d bitwise and d constant per instance the loop reproduces, bit for bit,
 * mpcx_lmpc_loop_create_observed given the same d as per-instance dmeas.  gain_batch is what mpcx_dare_batch (MPCX_DARE_ESTIMATOR, n = nx + ndu,
 * m = ny) writes for the augmented pair ([[A, Bd], [0, I]], [C, Dd]): hand it over as it is.  The augmented pair is detectable only where
 * rank [[I - A, -Bd], [C, Dd]] = nx + ndu, which needs ndu <= ny.  This loop computes no steady-state target from dhat: the output settles on its
 * reference where the input weight is zero (or the input reference is the steady-state input); with a non-zero input weight use
 * mpcx_lmpc_loop_create_offset_free_target below, which does.  The loop is an mpcx_lmpc_loop_t as before; gain is copied at creation; gain_batch, xhat0, dhat0 and meas_noise are read by
 * every run: refill them in place. */
typedef struct mpcx_lmpc_disturbance_observer_desc {
    const double *gain;                           /* HOST, column-major [(nx+ndu) x ny] (rows 0 .. nx-1 = Lx, then Ld): one gain for the batch, or NULL */
    const double *gain_batch;                     /* device, [B x (nx+ndu)*ny], per instance, column-major; excludes gain */
    const double *xhat0;                          /* device [B x nx] or NULL (= x0) */
    const double *dhat0;                          /* device [B x ndu] or NULL (= 0) */
    const double *meas_noise;                     /* device [ticks x B x ny] or NULL */
    double *traj_xhat, *traj_dhat, *traj_y;       /* device, optional: [(ticks+1) x B x nx], [(ticks+1) x B x ndu], [ticks x B x ny] */
} mpcx_lmpc_disturbance_observer_desc;
/* MPCX_E_INVALID, ahead of any look at the handle's state, for a null descriptor, for neither or both of gain / gain_batch, and for a controller
 * without exogenous inputs (ndu = 0: there is no disturbance model to estimate). */
int mpcx_lmpc_loop_create_offset_free(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o, void *stream, mpcx_lmpc_loop_t *out);
int mpcx_lmpc_disturbance_observer_desc_size(void);   /* sizeof(mpcx_lmpc_disturbance_observer_desc), for bindings that mirror the struct */
/* An offset-free loop with steady-state targets (no reference counterpart): with a non-zero input weight the input term of the cost pulls the
 * steady state away from yref unless the input reference is the steady-state input, so the loop computes that input from dhat at every tick,
 *     us_k = T [r_k; dhat_k; ubar_k],      T = [Tr | Td | Tu]  [nu x nrhs], nrhs = ny + ndu + nu, column-major: what mpcx_target_map_batch writes
 * and the solve of tick k reads the loop's own [B x nu] buffer us_k as its MPCX_REF_PER_INSTANCE uref (as it reads dhat_k for dmeas).  The loop
 * descriptor's uref, in every mode it has, becomes ubar_k: step 0 of the tick's array (a bank's "shared": each controller's own); r_k is step 0
 * of the tick's yref, taken the same way; yref still reaches the solve unchanged in every mode.  us_0 comes from dhat0, r_0, ubar_0 when a run
 * begins, us_{k+1} from the advance kernel of tick k; every row is summed from 0 with fused multiply-adds by ascending column (Tr, Td, Tu), the
 * sum of mpcx_target_apply_batch, bit for bit.  us is not clipped to the input bounds and yref is not replaced by a steady-state output: targets
 * under active bounds are a QP, which is out of scope -- traj_us shows what the solve was given.  map is copied at creation; map_batch is read
 * at the head of every run: refill it in place. */
typedef struct mpcx_lmpc_target_desc {
    const double *map;                            /* HOST, column-major [nu x nrhs]: one map for the batch, or NULL */
    const double *map_batch;                      /* device, [B x nu*nrhs], per instance, column-major; excludes map */
    double *traj_us;                              /* device, optional: [(ticks+1) x B x nu] */
} mpcx_lmpc_target_desc;
/* MPCX_E_INVALID, ahead of any look at the handle's state, for a null target descriptor, for neither or both of map / map_batch, and for
 * everything mpcx_lmpc_loop_create_offset_free refuses. */
int mpcx_lmpc_loop_create_offset_free_target(mpcx_lmpc_t h, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                             const mpcx_lmpc_target_desc *t, void *stream, mpcx_lmpc_loop_t *out);
int mpcx_lmpc_target_desc_size(void);             /* sizeof(mpcx_lmpc_target_desc), for bindings that mirror the struct */
/* The steady-state Kalman predictor gain of the controller's own (A, C) (no reference counterpart), on the host in doubles; works on a host-only
 * handle.  L = A P C' (C P C' + Rv)^-1 with P the fixed point of P <- A P A' - A P C' (C P C' + Rv)^-1 C P A' + Qw, iterated from P = Qw and
 * symmetrised every time, until the largest change of an entry is <= 1e-14 times the largest entry.  Qw [nx x nx], Rv [ny x ny], gain_out
 * [nx x ny], P_out [nx x nx] or NULL, all column-major; iterations (or NULL) receives the count.  MPCX_E_STATE without a model, MPCX_E_INVALID
 * for a Qw or Rv that is not symmetric or an Rv that is not positive definite, MPCX_E_NUMERIC when 100000 iterations have not converged (an
 * (A, C) that is not detectable, for instance). */
int mpcx_lmpc_kalman_gain(mpcx_lmpc_t h, const double *Qw, const double *Rv, double *gain_out, double *P_out, int *iterations);

/* Convenience for callers whose data lives in host memory (the reference's optimize(x0, lastU) is
 * such a caller): stages the inputs to HBM, runs mpcx_lmpc_solve_batch on the default stream, copies
 * the results back and synchronises.  References use the matrices given to the host setters.  Any
 * output pointer may be NULL except cmd.  seq_* are [B x (ph+1) x n] row-major, as in the batch struct. */
int mpcx_lmpc_solve_host(mpcx_lmpc_t h, int batch, const double *x0, const double *u0,
                         double *cmd, double *cost, int32_t *status, int32_t *solver_status, int32_t *is_feasible,
                         double *seq_state, double *seq_output, double *seq_input);

/* ---- introspection -------------------------------------------------------------- */
/* sizes of the reference QP (ProblemBuilder.hpp:70-76) and of the condensed one */
typedef struct mpcx_lmpc_info {
    int n_ref, m_ref, neq_ref;     /* reference QP variables / rows / equality rows          */
    int nz, mg;                    /* condensed: decision variables, general inequality rows */
    int active_words;              /* uint32 words per instance in active_lower/upper        */
    int kernel_variant;            /* which template instantiation serves these dimensions   */
    double flops_setup;            /* algorithmic flops of one set-up                         */
    double flops_per_admm_iter;    /* algorithmic flops of one ADMM iteration of one instance */
    double flops_fixed_per_solve;  /* assembly + unconstrained solve + cost, per instance     */
    double bytes_per_solve;        /* algorithmic HBM bytes per instance (inputs + outputs)   */
} mpcx_lmpc_info;
int mpcx_lmpc_get_info(mpcx_lmpc_t h, mpcx_lmpc_info *info);

/* ---- NLMPC transcription (rows a10-a20 of SURVEY.md 8) ---------------------------- */
/* What the reference computes inside every NLopt callback of NLOptimizer<> (NLOptimizer.hpp:760-997):
 * Mapping::unwrapVector (Mapping.hpp:174-211), Objective::evaluate + forward-difference gradient
 * (Objective.hpp:91-265), the dynamics equalities with their central-difference Jacobian blocks
 * (Constraints.hpp:490-628, 844-905) and the user inequalities with theirs (Constraints.hpp:211-316),
 * for a batch of decision vectors in one launch.  The reference's user hooks are host std::function
 * objects (IDimensionable.hpp:94-149); device code cannot call those.  The hooks are device code instead:
 * the reference's example systems are built in and picked by id (below); any other system comes in through
 * mpcx_nlmpc_create_custom (hooks compiled by the caller with hipcc, what mpc::NLMPC<>'s setters use) or
 * mpcx_nlmpc_create_from_source (hooks compiled at run time from the lambda bodies, what the Python front-end uses). */
typedef struct mpcx_nlmpc *mpcx_nlmpc_t;
enum { MPCX_MODEL_VANDERPOL = 1,   /* examples/vanderpol_ex.cpp: nx=2 nu=1, continuous, ineq u_i <= 0.5        */
       MPCX_MODEL_UGV = 2,         /* examples/ugv_ex.cpp: nx=4 nu=2, discrete, two circular obstacles           */
       MPCX_MODEL_OSCILLATORS6 = 3,/* examples/networked_oscillators_ex.cpp: 6 coupled oscillators, nx=12 nu=6   */
       MPCX_MODEL_OSCILLATORS8 = 4,/* the same network with 8 oscillators (BASELINE config 5), nx=16 nu=8        */
       MPCX_MODEL_VANDERPOL_TERMINAL = 5,/* Van der Pol + the user equality x(ph) = 0 (setEqConFunction path)    */
       MPCX_MODEL_VANDERPOL_RATE = 6 };/* Van der Pol + a rate limit |u_i - u_{i-1}| <= params[0] (default 0.1): inequality rows
                                          with two entries, several rows on one input (no reference example has them)  */
typedef struct mpcx_nlmpc_dims {
    int nx, nu, ph, ch;
    int nz;      /* decision variables  ph*nx + ch*nu + 1 (Objective.hpp:45)                         */
    int neq;     /* dynamics equalities ph*nx                                                         */
    int nineq;   /* user inequalities                                                                 */
    int jeq_w;   /* width of one equality Jacobian block row: 2*nx + nu                               */
    int neq_user;/* user equalities (NLMPC::setEqConFunction)                                         */
    int ny;      /* outputs (NLMPC::setOutputFunction; zeros in the sequence when the model has none)  */
    int nbnd;    /* finite state / input bounds: rows nineq + neq_user .. of the sub-problem (multipliers) */
    int n_params;/* model parameters of a built-in system = columns of mpcx_nlmpc_batch.params (0: hooks)  */
} mpcx_nlmpc_dims;
/* NLMPC::setDiscretizationSamplingTime / setStateSpaceFunction / setObjectiveFunction /
 * setIneqConFunction (NLMPC.hpp:108-214) for a built-in model; `params` (n doubles, may be NULL
 * for the model's defaults) are the constants its functors capture in the reference example.
 * UGV: [v_pref_x, v_pref_y, ox0, oy0, r0, ox1, oy1, r1, Ts].  Oscillators: [mu, k].  Van der Pol:
 * none (Ts is the collocation step).                                                             */
int mpcx_nlmpc_create(int model_id, int ph, int ch, double Ts, const double *params, int n_params,
                      int device, mpcx_nlmpc_t *out);
int mpcx_nlmpc_destroy(mpcx_nlmpc_t h);
int mpcx_nlmpc_get_dims(mpcx_nlmpc_t h, mpcx_nlmpc_dims *d);

/* ---- user hooks (NLMPC::setStateSpaceFunction / setOutputFunction / setObjectiveFunction / setIneqConFunction /
 * setEqConFunction, NLMPC.hpp:139-281; handle types IDimensionable.hpp:94-149) ----------------------------------------
 * The reference's hooks are host closures, which a kernel cannot call.  Two ways to give this library device code with the
 * same signatures instead of picking a built-in model:
 *
 * (1) compiled by the caller.  The engine is a header (include/mpcx/nlmpc_engine.hpp); a translation unit compiled with
 *     hipcc instantiates it for its own hook types (include/mpcx/nlmpc_hooks.hpp -- what mpc::NLMPC<>'s setters do in
 *     include/mpcx/NLMPC.hpp) and registers the two launch thunks here.  The library keeps owning the workspace, bounds,
 *     parameters and every entry point below; `hooks` (the closure objects, hooks_bytes of them) is copied to HBM and
 *     handed to the kernels.                                                                                           */
typedef struct mpcx_nlmpc_custom {
    int nx, nu, ny, ph, ch, nineq, neq_user;
    int has_output;        /* an output function was set (otherwise outputs read as zeros, Model.hpp:72-96)              */
    int vector_hooks;      /* 1: hooks with the reference's whole-vector signatures (mpcx::HookModel); 0: a zoo-style
                              model struct with component-wise constraints and declared structure                        */
    const void *hooks; int hooks_bytes;
    /* mpcx::engine::launch_evaluate<Model> / launch_solve<Model>; the struct arguments are mpcx::NlmpcDev,
     * mpcx::NlmpcBatchDev, mpcx::NlmpcSolveDev (include/mpcx/nlmpc_device.hpp), ctx is passed back unchanged          */
    int (*launch_evaluate)(void *ctx, const void *dev, const void *batch, void *stream);
    int (*launch_solve)(void *ctx, const void *dev, const void *solve, void *stream);
    void *launch_ctx;
} mpcx_nlmpc_custom;
/* Ts > 0: the state function is a vector field dx/dt and the transcription is trapezoidal collocation with step Ts
 * (NLMPC::setDiscretizationSamplingTime, NLMPC.hpp:80-90); Ts <= 0: the state function returns x(k+1).                  */
int mpcx_nlmpc_create_custom(const mpcx_nlmpc_custom *c, double Ts, int device, mpcx_nlmpc_t *out);

/* (2) compiled at run time (hipRTC).  The hooks are given as C++ source: each string is the BODY of the corresponding
 *     reference lambda, with these parameter names --
 *       state_fn      (dx, x, u, step)           fills dx (or the next state, Ts <= 0)          required
 *       objective_fn  (x, y, u, e)               returns the cost                               required
 *       ineq_fn       (in_con, x, y, u, e)       fills in_con, in_con <= 0                      NULL when nineq = 0
 *       eq_fn         (eq_con, x, u)             fills eq_con, eq_con = 0                       NULL when neq_user = 0
 *       output_fn     (y, x, u, step)            fills y                                        NULL: outputs are zeros
 *     with the reference's types (mpc::cvec<n>, mpc::mat<ph+1, n>, include/mpcx/matrix.hpp) and the constants num_states,
 *     num_inputs, num_output, pred_hor, ctrl_hor, ineq_c, eq_c in scope; `preamble` (may be NULL) is pasted before them at
 *     namespace scope (constants, helper __device__ functions).  Example, the reference's examples/vanderpol_ex.cpp:
 *       state_fn     "dx(0) = ((1.0 - (x(1) * x(1))) * x(0)) - x(1) + u(0); dx(1) = x(0);"
 *       objective_fn "return x.array().square().sum() + u.array().square().sum();"
 *       ineq_fn      "for (int i = 0; i < ineq_c; i++) in_con(i) = u(i, 0) - 0.5;"
 *     The compiler's log is available through mpcx_last_error() when compilation fails.  Needs libhiprtc.so.7.         */
typedef struct mpcx_nlmpc_source {
    int nx, nu, ny, ph, ch, nineq, neq_user;
    const char *preamble, *state_fn, *objective_fn, *ineq_fn, *eq_fn, *output_fn;
} mpcx_nlmpc_source;
int mpcx_nlmpc_create_from_source(const mpcx_nlmpc_source *src, double Ts, int device, mpcx_nlmpc_t *out);

/* NLMPC::setInputScale / setStateScale (NLMPC.hpp:108,123 -> Mapping::setInputScaling / setStateScaling, Mapping.hpp:71-86):
 * the hooks see U = input_scale * z_u and X = [x0; z_x] / state_scale (Mapping.hpp:174-211), and the Jacobians carry the
 * factors the reference gives them, including what it leaves out (no chain rule on the cost's state gradient,
 * Objective.hpp:107-144; inequality state columns multiplied, not divided, Constraints.hpp:269-284).  nu / nx doubles.   */
int mpcx_nlmpc_set_input_scale(mpcx_nlmpc_t h, const double *scaling);
int mpcx_nlmpc_set_state_scale(mpcx_nlmpc_t h, const double *scaling);
/* Device pointers, fp64.  z [B x nz] (layout [x_1..x_ph | u blocks (ch) | slack]), x0 [B x nx].
 * Any output may be NULL.  cost [B]; grad [B x nz]; ceq [B x neq]; cineq [B x (nineq + neq_user)]: the user
 * inequalities, then the user equalities (Constraints::evaluateEq, Constraints.hpp:365-442);
 * jineq [B x (nineq + neq_user) x nz] row-major (dense: a user constraint may depend on anything);
 * jeq [B x ph x nx x jeq_w] row-major blocks [dc_i/dx_i | dc_i/dx_{i+1} | dc_i/du_i] -- the
 * non-zeros of the reference's dense [neq x nz] Jacobian: block i sits in rows i*nx.., columns
 * (i-1)*nx.. (absent for i = 0, x_0 is data), i*nx.., ph*nx + min(i, ch-1)*nu...                */
int mpcx_nlmpc_evaluate_batch(mpcx_nlmpc_t h, int batch, const double *z, const double *x0,
                              double *cost, double *grad, double *ceq, double *jeq,
                              double *cineq, double *jineq, void *stream);

/* mpc::NLParameters (Types.hpp:99-144), field for field.  The iteration stops when the largest step component falls below
 * 1e-6 * max(1, |z|_inf) with the dynamics defects below 1e-8 (solver_status 4), or when the line search finds no decrease
 * (finite-difference noise floor).  Positive tolerances add nlopt's own rules (set_ftol_rel / set_ftol_abs / set_xtol_rel /
 * set_xtol_abs, NLOptimizer.hpp:135-138, unit x weights :140), tested like SLSQP tests them, after a step that ends at a
 * feasible point: |f - f_prev| < absolute_ftol or < relative_ftol * (|f| + |f_prev|) / 2 -> solver_status 3 (FTOL_REACHED);
 * sum |dz| <= relative_xtol * sum |z| or every |dz_i| < absolute_xtol -> 4 (XTOL_REACHED).  Negative (the reference's
 * default): disabled.                                                                                              */
typedef struct mpcx_nlparams {
    int maximum_iteration;    /* 100 */
    double time_limit;        /* 0, accepted and ignored */
    int enable_warm_start;    /* 0; warm starts are driven by mpcx_nlmpc_batch.z_warm */
    double relative_ftol, relative_xtol, absolute_ftol, absolute_xtol;   /* -1 */
    int hard_constraints;     /* 1: slack fixed at zero (NLOptimizer.hpp:182-186) */
} mpcx_nlparams;
void mpcx_nlparams_default(mpcx_nlparams *p);
/* NLMPC::setOptimizerParameters -> NLOptimizer::setParameters (NLOptimizer.hpp:129-195) */
int mpcx_nlmpc_set_optimizer_parameters(mpcx_nlmpc_t h, const mpcx_nlparams *p);

/* NLMPC::setStateBounds / setInputBounds, vector + HorizonSlice form (NLMPC.hpp:346-398 -> NLOptimizer.hpp:346-404):
 * box bounds on the states x_1..x_ph (slice over the prediction horizon) and on the input blocks (slice over the
 * control horizon); {-1,-1} = the whole horizon.  They become rows of the sub-problem.  A starting point outside
 * them is moved to (ub - lb) / 2 as NLOptimizer::fixOptimalSolution does (NLOptimizer.hpp:705-716).  Output bounds
 * do not exist for NLMPC (NLMPC.hpp:318-325 throws).                                                        */
int mpcx_nlmpc_set_state_bounds_slice(mpcx_nlmpc_t h, const double *lo, const double *hi, int start, int end);
int mpcx_nlmpc_set_input_bounds_slice(mpcx_nlmpc_t h, const double *lo, const double *hi, int start, int end);

/* One batched NLOptimizer::run (NLOptimizer.hpp:412-638).  Device pointers.  Outputs other than
 * cmd may be NULL.  status uses MPCX_STATUS_* (ResultStatus), solver_status nlopt's result codes
 * (3 FTOL_REACHED, 4 XTOL_REACHED, 5 MAXEVAL_REACHED, -1 FAILURE = inconsistent linearised constraints,
 * -3 OUT_OF_MEMORY = more than 128 rows active at once, -4 ROUNDOFF_LIMITED = line search stalled far from a solution,
 * -5 FORCED_STOP = the kernel's own consistency guard tripped: a wavefront reached a phase boundary with lanes missing -- never seen, tests assert it) as mapped at NLOptimizer.hpp:729-750; on failure
 * cmd = u0 and cost = inf as at :613-624.  is_feasible = every user inequality <= 1e-10 and every user
 * equality within 1e-10 (Constraints.hpp:157-202, tolerances NLMPC.hpp:166, 262).                 */
typedef struct mpcx_nlmpc_batch {
    int batch;
    const double *x0;          /* [B x nx] */
    const double *u0;          /* [B x nu] */
    const double *z_warm;      /* [B x nz] previous solutions, shifted one step on entry as at
                                  NLOptimizer.hpp:460-510; NULL = cold start (:431-451)            */
    double *cmd;               /* [B x nu] */
    double *cost;              /* [B] */
    int32_t *status, *solver_status, *is_feasible, *iterations;   /* [B] each */
    double *z;                 /* [B x nz] the optimal decision vectors (next call's z_warm; may be the
                                  same buffer as this call's z_warm: an instance reads its start
                                  before its result is written)                                     */
    double *seq_state;         /* [B x (ph+1) x nx] row-major, row 0 = x0                           */
    double *seq_input;         /* [B x (ph+1) x nu]                                                 */
    double *seq_output;        /* [B x (ph+1) x ny] Model::getOutput (Model.hpp:72-96)                */
    int warm_curvature;        /* extension, with z_warm only: 1 = also keep the curvature estimate the previous solve of
                                  the same batch left in the handle's workspace (NLopt restarts its BFGS matrix on every
                                  optimize(); the optimum is the same, the iterations are fewer)                   */
    double *multipliers;       /* extension, may be NULL: [B x (nineq + neq_user + nbnd)] multipliers of the last quadratic
                                  sub-problem -- user inequalities, user equalities, then the finite bounds in the order
                                  (index into z ascending; upper before lower); non-zero = in the active set        */
    const double *params;      /* extension, may be NULL: [B x n_params] -- every instance its own parameters of the built-in
                                  system (the constants the reference example's closures capture: each UGV its own obstacles
                                  and preferred velocity, each oscillator network its own mu and coupling), in the order of
                                  mpcx_nlmpc_create's `params`.  NULL: the controller's parameters for all.  Not for hook
                                  models (their constants live in the closures).                                     */
} mpcx_nlmpc_batch;
int mpcx_nlmpc_solve_batch(mpcx_nlmpc_t h, const mpcx_nlmpc_batch *b, void *stream);
/* The same for callers whose data lives in host memory (the reference's optimize(x0, lastU) is such a caller): stages,
 * solves on the default stream, copies back, synchronises.  Outputs other than cmd may be NULL; z_warm may be NULL. */
int mpcx_nlmpc_solve_host(mpcx_nlmpc_t h, int batch, const double *x0, const double *u0, const double *z_warm, double *cmd,
                          double *cost, int32_t *status, int32_t *solver_status, int32_t *is_feasible, int32_t *iterations,
                          double *z, double *seq_state, double *seq_input);
/* `repeats` back-to-back launches bracketed by HIP events on `stream`; mean milliseconds. */
int mpcx_nlmpc_time_solve_batch(mpcx_nlmpc_t h, const mpcx_nlmpc_batch *b, void *stream, int repeats, float *ms_mean);

/* ---- NLMPC closed loop on the device ------------------------------------------------------------------------------------
 * The caller's loop of the reference examples (examples/vanderpol_ex.cpp:76-85, ugv_ex.cpp: `for (;;) { res = optimize(x, lastU);
 * lastU = res.cmd; x = plant(x, res.cmd); }`) for a batch, with no host work between two solves: a tick is mpcx_nlmpc_solve_batch on
 * the loop's own x / u / z buffers followed by an advance kernel that steps the plant, hands the command over as the next lastU and
 * files the tick's row of every trajectory.  A tick is captured once as a HIP graph (a linear chain on one stream) and a run replays it
 * `ticks` times; the tick number lives on the device.  Built-in systems only: a hook model (mpcx_nlmpc_create_custom,
 * mpcx_nlmpc_create_from_source) gets MPCX_E_UNSUPPORTED from mpcx_nlmpc_loop_create and mpcx_nlmpc_plant_step_batch -- loops for
 * hook models come later.
 * The plant is the controller's own state function: x <- f(x, cmd, p) for a discrete model (UGV, ugv_ex.cpp), `substeps` forward-Euler
 * steps x <- x + (Ts / substeps) f(x, cmd, p) for a continuous one (substeps = 1 is vanderpol_ex.cpp:79-80), then x += w_k where a noise
 * array is given.  p is the instance's row of plant_params, else its row of params, else the controller's parameters.  States and
 * commands are in physical units (the Mapping scalings act inside the solve only).  On a failed solve cmd is already u0 (see
 * mpcx_nlmpc_batch), which the plant then holds. */
typedef struct mpcx_nlmpc_loop *mpcx_nlmpc_loop_t;
typedef struct mpcx_nlmpc_loop_desc {
    int batch, ticks;
    const double *x0, *u0;          /* device [B x nx], [B x nu]; read again by every run */
    const double *params;           /* device [B x n_params] or NULL: per-instance controller parameters (as mpcx_nlmpc_batch.params) */
    const double *plant_params;     /* device [B x n_params] or NULL: the plant's parameters where they differ from the controller's */
    const double *noise;            /* device [ticks x B x nx] or NULL */
    int substeps;                   /* Euler sub-steps of a continuous plant per tick, >= 1 (1 = the reference example); ignored for discrete models */
    int warm;                       /* 1: ticks >= 1 start from the shifted previous solution with the carried curvature estimate; tick 0 is cold */
    double *traj_x, *traj_u;        /* device, required: [(ticks+1) x B x nx], [ticks x B x nu], tick-major */
    double *traj_cost; int32_t *traj_status, *traj_solver_status, *traj_is_feasible, *traj_iterations;   /* optional */
} mpcx_nlmpc_loop_desc;
/* The loop of examples/vanderpol_ex.cpp:76-85 / ugv_ex.cpp, prepared: allocates the loop's buffers, runs one plain tick on `stream` (a
 * non-default stream; that sizes the SQP workspace and uploads pending bounds), synchronises it and captures tick 0 (cold) and, with
 * warm and ticks > 1, every later tick as a second graph.  The graphs hold the controller's workspace, bounds, scalings, optimizer
 * parameters and tolerances as they were: after any setter of the controller, or a plain solve of a larger batch (it re-allocates the
 * workspace), mpcx_nlmpc_loop_run returns MPCX_E_STATE -- create a new loop.  Destroy a loop before its controller. */
int mpcx_nlmpc_loop_create(mpcx_nlmpc_t h, const mpcx_nlmpc_loop_desc *d, void *stream, mpcx_nlmpc_loop_t *out);
/* One run of that loop (examples/vanderpol_ex.cpp:76-85 / ugv_ex.cpp), asynchronous: x <- x0, u <- u0, then `ticks` graph launches on
 * `stream`.  The trajectories are complete once the stream has been synchronised.  One launch or run of a controller in flight at a time
 * (they share its workspace); a plain solve after a run takes no curvature estimate over from it. */
int mpcx_nlmpc_loop_run(mpcx_nlmpc_loop_t l, void *stream);
int mpcx_nlmpc_loop_destroy(mpcx_nlmpc_loop_t l);
int mpcx_nlmpc_loop_desc_size(void);            /* sizeof(mpcx_nlmpc_loop_desc) as the library was built: for bindings that mirror it */
/* The plant step of that loop alone (the `x = plant(x, res.cmd)` line of examples/vanderpol_ex.cpp:79-80 / ugv_ex.cpp) for callers who
 * drive the loop themselves: x_next [B x nx] from x, u [B x nu], per-instance params [B x n_params] or NULL (the controller's) and
 * noise [B x nx] or NULL; x_next may be x.  The same device function as the loop's advance kernel: the two agree bit for bit. */
int mpcx_nlmpc_plant_step_batch(mpcx_nlmpc_t h, int batch, const double *x, const double *u, const double *params,
                                const double *noise /* [B x nx] or NULL */, int substeps, double *x_next, void *stream);

/* ---- NLMPC closed loop with output feedback: an extended Kalman filter in the advance step ---------------------------------
 * An observed loop carries the truth x, the estimate xhat and its covariance P [nx x nx] per instance.  The estimate is the loop's
 * state buffer: the solve of tick k reads xhat_k, and the descriptors of the solve are untouched.  With Phi the noise-free plant
 * step above, the advance kernel of tick k computes, all from tick-k data,
 *   x_{k+1}    = Phi(x_k, cmd_k, p_plant) + w_k             as in the unobserved loop (plant_params, else params, else the controller's)
 *   y_{k+1}    = Cm x_{k+1} + v_k                           v: meas_noise
 *   xhat-      = Phi(xhat_k, cmd_k, p_ctrl)                 p_ctrl: the instance's row of params, else the controller's -- never plant_params
 *   F[:, j]    = (Phi(xhat_k + h_j e_j) - Phi(xhat_k - h_j e_j)) / (x+_j - x-_j),  h_j = 2^-17 max(1, |xhat_k,j|); the divisor is the
 *                difference of the two perturbed values as stored, not 2 h_j
 *   P-         = F P_k F' + Q;   S = Cm P- Cm' + R;   K = P- Cm' S^-1 (Cholesky of S)
 *   xhat_{k+1} = xhat- + K (y_{k+1} - Cm xhat-)
 *   P_{k+1}    = sym((I - K Cm) P- (I - K Cm)' + K R K')    Joseph form, then (P + P') / 2
 * States are in physical units.  If a pivot of S is not > 0 or not finite (tested before the square root and any division), the
 * update of that tick is skipped: xhat_{k+1} = xhat-, P_{k+1} = sym(P-), and bit 0 of the instance's ekf_flags word is set; every
 * run clears the flags first.  No NaN is written on that account and the loop goes on.
 * Cm, Q, R, P0 are HOST arrays, column-major, one for the batch, copied at creation; Cm = NULL is the identity with ny = nx.  Built-in
 * systems only (hook models: MPCX_E_UNSUPPORTED); the measurement is linear; per-instance Q / R / P0 and unscented or iterated filters
 * are not provided. */
typedef struct mpcx_nlmpc_ekf_desc {
    int ny;                         /* measurements per instance, 1 .. nx */
    const double *Cm;               /* host [ny x nx] or NULL (identity, ny = nx) */
    const double *Q, *R, *P0;       /* host [nx x nx], [ny x ny], [nx x nx] */
    const double *xhat0;            /* device [B x nx] or NULL (x0); read again by every run */
    const double *meas_noise;       /* device [ticks x B x ny] or NULL; read again by every run */
    double *traj_xhat, *traj_y;     /* device, required: [(ticks+1) x B x nx] (row 0 = xhat0), [ticks x B x ny] (row k = y_{k+1}) */
    double *traj_P;                 /* device [(ticks+1) x B x nx nx] or NULL */
    int32_t *ekf_flags;             /* device [B] or NULL */
} mpcx_nlmpc_ekf_desc;
/* mpcx_nlmpc_loop_create with the filter `e` in the advance step.  `d` means what it means there (traj_x is the truth); the loop is
 * the same type: mpcx_nlmpc_loop_run, _destroy and the debug calls serve it, `warm` and the invalidation by a setter are unchanged. */
int mpcx_nlmpc_loop_create_observed(mpcx_nlmpc_t h, const mpcx_nlmpc_loop_desc *d, const mpcx_nlmpc_ekf_desc *e, void *stream,
                                    mpcx_nlmpc_loop_t *out);
int mpcx_nlmpc_ekf_desc_size(void);             /* sizeof(mpcx_nlmpc_ekf_desc) as the library was built */
/* The filter step of that loop alone, the sibling of mpcx_nlmpc_plant_step_batch for callers who drive the loop themselves: from device
 * xhat [B x nx], P [B x nx nx], u [B x nu] and the measurement y [B x ny] of the new state to device xhat_next, P_next and flags [B]
 * (0, or 1 where the update was skipped); xhat_next may be xhat and P_next may be P.  params: device [B x n_params] or NULL (the
 * controller's); Cm (or NULL), Q, R: host, as above.  The same device function as the observed loop's advance kernel: the two agree bit
 * for bit.  The matrices are staged through a buffer of the controller: one call of a controller in flight at a time. */
int mpcx_nlmpc_ekf_step_batch(mpcx_nlmpc_t h, int batch, const double *xhat, const double *P, const double *u, const double *y,
                              const double *params, const double *Cm, const double *Q, const double *R, int ny, int substeps,
                              double *xhat_next, double *P_next, int32_t *flags, void *stream);

/* ---- set-up utility -------------------------------------------------------- */
/* mpc::discretization<nx, nu>(A, B, Ts, Ad, Bd) (Utils.hpp:23-47) for a batch of continuous-time models on the
 * device: [Ad Bd; 0 I] = exp([[A B]; [0 0]] Ts).  Device pointers, column-major matrices per instance
 * (A [B x nx x nx], B [B x nx x nu]); Ts one value (ts_per_instance = 0) or [B].  The variant with a
 * disturbance matrix (Utils.hpp:63-89) is the same call with Be appended to B's columns.  nx + nu <= 48.   */
int mpcx_discretize_batch(int device, int nx, int nu, int batch, const double *A, const double *B, const double *Ts,
                          int ts_per_instance, double *Ad, double *Bd, void *stream);

/* A batch of discrete algebraic Riccati equations on the device (no reference counterpart; kernel dare_sda of dare_kernels.hip, a
 * structure-preserving doubling iteration, one equation per wavefront):
 *   MPCX_DARE_CONTROL    X = A'XA - A'XB (R + B'XB)^-1 B'XA + Q,  gain K = (R + B'XB)^-1 B'XA [m x n]; BorC is B [n x m]
 *   MPCX_DARE_ESTIMATOR  P = APA' - APC' (CPC' + R)^-1 CPA' + Q,  gain L = APC' (CPC' + R)^-1 [n x m]; BorC is C [m x n]
 * The estimator gain is the predictor gain of mpcx_lmpc_observer_desc and is written in gain_batch's layout: hand it over as it is.
 * Device pointers, column-major matrices per instance: A [B x n x n], BorC [B x n m], Q [n x n] and R [m x m] one for the batch or
 * (q_per_instance, r_per_instance) one per instance, both symmetric (their symmetric parts are used); X [B x n x n]; gain [B x n m],
 * flags [B] and iterations [B] (the doublings taken) may each be NULL.  1 <= n <= 32, 1 <= m <= 32 (m may exceed n).
 * flags: 0 converged; 1 R is not positive definite; 2 no convergence within 40 doublings; 3 a non-finite value, a vanishing pivot or a
 * failed Cholesky factorisation of R + B'XB during the iteration (an unstable mode that BorC does not reach ends here).  An instance
 * with a non-zero flag has NaN in every entry of X and of its gain; the others are not affected, and an instance's bits depend on its
 * own inputs alone.  MPCX_E_INVALID for another form, sizes outside the limits, a negative batch or a null A, BorC, Q, R or X: checked
 * before anything touches a device. */
#define MPCX_DARE_CONTROL   0
#define MPCX_DARE_ESTIMATOR 1
int mpcx_dare_batch(int device, int form, int n, int m, int batch, const double *A, const double *BorC, const double *Q, const double *R,
                    int q_per_instance, int r_per_instance, double *X, double *gain, int32_t *flags, int32_t *iterations, void *stream);

/* A batch of steady-state target maps on the device (no reference counterpart; kernel target_map of target_kernels.hip, one instance per
 * wavefront).  For a model (A, B, Bd, C, Dd) the target of a reference r, a disturbance estimate dhat and an input reference ubar is
 *     minimise 1/2 |us - ubar|^2   subject to   (I - A) xs - B us = Bd dhat,   C xs = r - Dd dhat
 * and linear in them: us = map_u [r; dhat; ubar], xs = map_x [r; dhat; ubar].  The maps come from the KKT system of order 2 nx + nu + ny by Gaussian
 * elimination with partial pivoting.  Device pointers, column-major per instance: A [B x nx nx], B [B x nx nu], Bd [B x nx ndu], C [B x ny nx],
 * Dd [B x ny ndu]; map_u [B x nu nrhs] with nrhs = ny + ndu + nu (the layout mpcx_lmpc_target_desc.map_batch takes); map_x [B x nx nrhs] and
 * flags [B] may be NULL.  flags: 0 fine; 1 singular (a vanishing or non-finite pivot: a reference that cannot be reached -- ny > nu, or a rank
 * deficient [[I - A, -B], [C, 0]] -- or an integrator the outputs do not see).  An instance with a non-zero flag has NaN in every entry of its
 * maps; the others are not affected, and an instance's bits depend on its own inputs alone.  MPCX_E_INVALID for nx, nu, ny < 1, ndu < 0, a
 * negative batch or a null A, B, C, map_u (Bd, Dd with ndu > 0); MPCX_E_UNSUPPORTED where the augmented matrix -- (2 nx + nu + ny) (2 nx + 2 nu
 * + 2 ny + ndu) doubles -- exceeds the LDS a workgroup may request: both checked before anything touches a device. */
int mpcx_target_map_batch(int device, int nx, int nu, int ndu, int ny, int batch, const double *A, const double *B, const double *Bd, const double *C,
                          const double *Dd, double *map_u, double *map_x, int32_t *flags, void *stream);
/* us[b] = map_u[b, or the one map] [r_b; dhat_b; ubar_b] for host-driven loops: every row summed from 0 with fused multiply-adds by ascending
 * column, by the device function the closed loop uses (bit-identical to it).  Device pointers: map_u [B x nu nrhs] (map_per_instance) or
 * [nu nrhs], r [B x ny], dhat [B x ndu], ubar [B x nu], us [B x nu]. */
int mpcx_target_apply_batch(int device, int nu, int ndu, int ny, int batch, const double *map_u, int map_per_instance, const double *r,
                            const double *dhat, const double *ubar, double *us, void *stream);

/* ---- multi-GPU: the one collective on the path --------------------------------- */
/* The reference solves one controller per object and has no coupling between objects (LMPC.hpp:751), so a batch shards
 * as contiguous slices, one process per GPU, and nothing is exchanged during the solve.  Afterwards every rank
 * contributes its block of optimal controls and receives everybody's: one RCCL ncclAllGather of doubles over xGMI.
 * mpcx_comm_* wraps the communicator so that a C++ host needs neither rccl.h nor PyTorch: rank 0 calls
 * mpcx_comm_get_unique_id, ships the MPCX_COMM_ID_BYTES bytes to the other ranks by any means (file, socket, MPI,
 * torch.distributed store), then every rank calls mpcx_comm_create (collective).  RCCL is bound at run time
 * (librccl.so.1); without it these calls return MPCX_E_DEVICE.                                                      */
#define MPCX_COMM_ID_BYTES 128
typedef struct mpcx_comm *mpcx_comm_t;
int mpcx_comm_get_unique_id(void *id_out /* MPCX_COMM_ID_BYTES bytes */);
int mpcx_comm_create(int device, int rank, int world, const void *id, mpcx_comm_t *out);
int mpcx_comm_destroy(mpcx_comm_t c);
int mpcx_comm_rank(mpcx_comm_t c);
int mpcx_comm_world(mpcx_comm_t c);
/* u_local [rows_per_rank x nu] -> u_all [world x rows_per_rank x nu], device pointers, every rank the same
 * rows_per_rank (ragged shards: pad the local block to the largest shard, libmpc_amd/distributed.py shows how).
 * Enqueued on `stream` -- pass the stream of the preceding mpcx_*_solve_batch so that the collective starts when the
 * solve retires, with no host synchronisation in between.  u_all may not alias u_local.                              */
int mpcx_allgather_u(mpcx_comm_t c, const double *u_local, int rows_per_rank, int nu, double *u_all, void *stream);

/* ---- heterogeneous batches (every instance its own model) ------------------------------------------
 * In the reference every controller object owns its model, weights and bounds (LMPC.hpp:751; ProblemBuilder.hpp:184-211,
 * 642-825).  A bank is K configured controllers (host-only handles are enough) with the same dimensions and the same pattern
 * of finite bounds, solved together: instance b of a batch uses controller model_index[b] (device array; NULL: controller b,
 * batch = K).  "Shared" references mean each controller's own setReferences / setExogenousInputs values.  The bank copies what
 * it needs: the controllers may be destroyed or changed afterwards (changes do not reach the bank).
 * Preconditions the library does not check on the device: every model_index[b] lies in [0, K) (an index outside reads another
 * controller's -- or no -- factors); a HIP graph captured from a solve holds the handle's workspace pointers, which a later solve
 * with a LARGER batch re-allocates: re-capture after growing the batch.
 * Set-up errors name the controller: MPCX_E_NUMERIC (its condensed Hessian or ADMM matrix does not factor), MPCX_E_INVALID (its
 * constraint structure differs from controller 0's, e.g. a constraint row that does not depend on the inputs in one of the two). */
typedef struct mpcx_lmpc_hetero *mpcx_lmpc_hetero_t;
int mpcx_lmpc_hetero_create(const mpcx_lmpc_t *controllers, int count, int device, mpcx_lmpc_hetero_t *out);
/* condense_on_host = 1: every controller's prediction matrices, Hessian, factors and dual Hessian on the host cores (what a single
 * controller's set-up does); 0: on the device, one workgroup per controller, the products on the f64 matrix pipe (falls back to the
 * host when the condensed problem exceeds 96 variables / the kernel's LDS plan)                                                 */
int mpcx_lmpc_hetero_create_ex(const mpcx_lmpc_t *controllers, int count, int device, int condense_on_host, mpcx_lmpc_hetero_t *out);
int mpcx_lmpc_hetero_destroy(mpcx_lmpc_hetero_t f);
int mpcx_lmpc_hetero_get_info(mpcx_lmpc_hetero_t f, int *count, int *active_words, int *m_ref, double *bytes_per_model);
int mpcx_lmpc_hetero_solve_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_batch *b, const int32_t *model_index, void *stream);
int mpcx_lmpc_hetero_time_solve_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_batch *b, const int32_t *model_index, void *stream,
                                      int repeats, float *ms_mean);
/* Sensitivities of a solved batch of a bank: what mpcx_lmpc_sensitivity_batch gives for one controller, every instance on its
 * own.  Replaces no call of the reference: the reference has no derivative.  The descriptor is mpcx_lmpc_sens unchanged -- modes, layouts, flags
 * and the NaN rule as documented there; active_lower / active_upper are the words mpcx_lmpc_hetero_solve_batch wrote.  model_index as in
 * mpcx_lmpc_hetero_solve_batch (device, [B]; NULL: instance b is controller b, batch = K); an index outside [0, K) gets flag 1.  d_yref is the
 * derivative with respect to a shift, common to all steps, of the output reference the instance was solved with -- the controller's own, per
 * instance or per step.  Asynchronous on `stream`; allocates nothing.  MPCX_E_INVALID: null bank or descriptor, batch below 1, missing active
 * words, unknown mode, a vector-Jacobian product without a seed, no model_index and a batch that is not the bank; MPCX_E_UNSUPPORTED: not even a
 * working set of one row fits the kernel's LDS plan. */
int mpcx_lmpc_hetero_sensitivity_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_sens *s, const int32_t *model_index, void *stream);
/* Gradients of a solved batch of a bank with respect to the weights, the bounds and the model of the controller each instance was solved with
 * (DESIGN.md 4.10b): what mpcx_lmpc_param_sensitivity_batch and mpcx_lmpc_model_sensitivity_batch give for one controller, in one launch, every
 * instance on its own controller; a second small launch adds the instances of each controller up.  One seed per instance (seed_cmd [B x nu] and /
 * or seed_input [B x (ph+1) x nu], as MPCX_SENS_VJP takes them).
 *   solved      the descriptor mpcx_lmpc_hetero_solve_batch filled, unchanged since: x0, u0, the references in their modes (MPCX_REF_SHARED:
 *               each controller's own), seq_output, seq_input, active_lower, active_upper (all required), seq_state (required where a model
 *               output is asked for) and status (optional: an unsolved instance gets flag 1).  The bank cannot tell whether the descriptor is
 *               the one it solved: that is the caller's to keep
 *   d_*         per instance: d_oweight [B x (ny x ph)], d_uweight, d_duweight [B x (nu x ph)], d_lower, d_upper [B x m_ref], d_A [B x (nx x nx)],
 *               d_B, d_C, d_Bd, d_Dd, every matrix column-major as its setter takes it; layouts, the rules of the bound rows and what is not
 *               differentiated as documented at mpcx_lmpc_param_sens and mpcx_lmpc_model_sens.  With d_A .. d_Dd all NULL the model part does
 *               not run at all; d_Bd / d_Dd (and c_Bd / c_Dd) are ignored without exogenous inputs
 *   c_*         per controller, [K x ..]: row k is the sum of the d_* rows of controller k's instances whose flag is 0, added in the order of
 *               group_order[group_offsets[k] .. group_offsets[k+1]) without floating-point atomics (two launches give the same bits); n_used [K]
 *               counts them.  group_order [B] and group_offsets [K+1] are the stable grouping of the instances by controller.  The sums read the
 *               per-instance rows: a c_* needs its d_*; whether an instance counts is read from flags, where given, else from its rows
 *   flags       the codes of mpcx_lmpc_sens -- 0 fine, 1 not solved or a model index outside [0, K), 2 dependent working set, 3 beyond the LDS
 *               plan; every requested d_* row of a flagged instance is NaN
 * All pointers are device pointers, every output may be NULL and is then written nowhere.  model_index as in mpcx_lmpc_hetero_solve_batch.
 * Asynchronous on `stream`; allocates nothing.  MPCX_E_INVALID: null bank or descriptor, no solved batch, batch below 1, neither seed, a required
 * member of `solved` missing, no model_index and a batch that is not the bank, a c_* without its d_* or without the group arrays, n_used without
 * the group arrays or without flags and any d_*; MPCX_E_UNSUPPORTED: not even a working set of one row fits the kernel's LDS plan. */
typedef struct mpcx_lmpc_bank_grad {
    const mpcx_lmpc_batch *solved;
    const double *seed_cmd, *seed_input;          /* at least one */
    double *d_oweight, *d_uweight, *d_duweight, *d_lower, *d_upper;
    double *d_A, *d_B, *d_C, *d_Bd, *d_Dd;
    int32_t *flags;                               /* optional [B] */
    const int32_t *group_order, *group_offsets;   /* [B], [K+1]; required iff any c_* or n_used is set */
    double *c_oweight, *c_uweight, *c_duweight, *c_lower, *c_upper, *c_A, *c_B, *c_C, *c_Bd, *c_Dd;
    int32_t *n_used;                              /* optional [K] */
} mpcx_lmpc_bank_grad;
int mpcx_lmpc_hetero_gradient_batch(mpcx_lmpc_hetero_t f, const mpcx_lmpc_bank_grad *g, const int32_t *model_index, void *stream);
int mpcx_lmpc_bank_grad_size(void);    /* sizeof(mpcx_lmpc_bank_grad) */
/* The closed loop of a bank: a tick is mpcx_lmpc_hetero_solve_batch on the loop's own buffers followed by the advance kernel, captured as for a
 * controller (two graphs with carry_working_set).  The loop is the type mpcx_lmpc_loop_create returns: mpcx_lmpc_loop_run, _destroy, _debug_replay
 * and _debug_tick serve both.  The descriptor's rules are mpcx_lmpc_loop_create's; without a model_index the batch must be the bank.  model_index
 * (device, [B] or NULL) is baked into the graph like the descriptor's pointers.  The plant: plant_batch if given; else plant_A, plant_B and
 * plant_Bd (all of them: a bank has no one model to complete a partial plant with), one plant for all; else each instance's own controller --
 * its A, B, Bd as the bank holds them -- through the per-instance advance kernel.  dmeas in MPCX_REF_SHARED mode drives each instance's plant
 * with step 0 of its own controller's exogenous input.  A bank has no setters, so nothing invalidates its loops; destroy a loop BEFORE its bank
 * (the graphs point into the bank's memory). */
int mpcx_lmpc_hetero_loop_create(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out);
/* The same with an observer (no reference counterpart): instance b is estimated with the model of its controller model_index[b], as the bank holds
 * it.  The controllers of a bank differ, so one gain for all is refused: gain_batch is required (MPCX_E_INVALID for gain). */
int mpcx_lmpc_hetero_loop_create_observed(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_observer_desc *o, const int32_t *model_index,
                                          void *stream, mpcx_lmpc_loop_t *out);
/* The offset-free loop of a bank: instance b is estimated with the model and the disturbance model of its controller; gain_batch is required
 * (MPCX_E_INVALID for gain, as above).  dmeas in MPCX_REF_SHARED mode: each controller's own exogenous input, step 0, as the true disturbance. */
int mpcx_lmpc_hetero_loop_create_offset_free(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                             const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out);
/* ... and with steady-state targets: a bank's controllers differ, so map_batch is required (MPCX_E_INVALID for map, ahead of any look at the
 * bank).  uref and yref in MPCX_REF_SHARED mode: each controller's own references, step 0, as ubar and r. */
int mpcx_lmpc_hetero_loop_create_offset_free_target(mpcx_lmpc_hetero_t f, const mpcx_lmpc_loop_desc *d, const mpcx_lmpc_disturbance_observer_desc *o,
                                                    const mpcx_lmpc_target_desc *t, const int32_t *model_index, void *stream, mpcx_lmpc_loop_t *out);

/* Sharding: this handle solves contiguous shards of a batch of `total` instances -- the kernel form is chosen for
 * the whole batch's size, so that a shard's results are bit for bit the rows of the unsharded solve (0 = every call is a whole batch). */
int mpcx_lmpc_set_total_batch(mpcx_lmpc_t h, int total);

/* ---- profiling and testing aids ------------------------------------------------------------------------------------
 * Not part of the reference-facing surface, but part of the exported ABI: bench.py's roofline block, tools/ and tests/ call
 * them, so they are declared (and kept) here.  "debug" in a name = may change between versions.                        */
/* mean time (ms) of [0] the assemble kernel, [1] the solve kernel, [2] the ADMM fallback kernel of one batch, each timed alone
 * with HIP events on `stream` over `repeats` launches (one-kernel forms: [0] = 0, [1] = the whole step's kernel; controllers whose
 * cost comes from its definition -- "flags"[0] below -- : [1] = lmpc_solve + lmpc_cost_mfma, launched back to back)                */
int mpcx_lmpc_debug_time_kernels(mpcx_lmpc_t h, const mpcx_lmpc_batch *b, void *stream, int repeats, float *ms3);
/* condensed arrays of the host set-up by name ("H", "Kinv", "Gr", "Gc", "Y", "lw", "uw", "rho_b", "lg0", "ug0", "rho_g", "dims",
 * "dims_maps", "MA0", "MA1", "g_refrow", "g_step", "g_kind", "g_comp", "flags" = [cost from its definition, one-workgroup form
 * available, fused mat-vec form available], "fallback" = [instances the fallback kernel served in the last step that left it any (reading
 * clears it), entries the failure queue holds, wavefronts of the fallback kernel's grid], "terminal" = the stored terminal cost
 * [P | xT | Tx], P symmetrised, empty without one, "wOutput" / "wU" = the output and input weights as stored, [ny | nu x (ph + 1)] column-major,
 * user column k in internal column k + 1, "MF1" = the composed map [rowsF x kin] column-major, "dims_fused" = [rowsF, nsp, kin, nxp, nup,
 * nyp, ione], "boxrow_ptr" / "boxrow_ref" = the CSR table variable -> reference rows, "blk" = the condensed block of every step,
 * "Cq" = the derivative of the outputs of the steps 1 .. ph with respect to the decision vector, [rows16 x nz] column-major, rows16 = ny ph
 * rounded up to 16, row (i - 1) ny + a = output a of step i);
 * out = NULL returns the length                                                                                                               */
int mpcx_lmpc_debug_get(mpcx_lmpc_t h, const char *name, double *out, int cap);
/* how many full set-ups (condensing + device rebuild) and how many reference-only refreshes have run on this handle */
int mpcx_lmpc_debug_setup_counts(mpcx_lmpc_t h, int *full, int *refs);
/* solve path: 0 = assemble and solve as two kernels; 1 = the record computed inside the solve kernel by one mat-vec (persistent
 * form from 1024 instances on); 2 = assemble + solve in one workgroup of sixteen wavefronts; -1 = automatic (the default: the
 * workgroup form up to 4096 instances, two kernels beyond; the fused forms only on request)                                   */
int mpcx_lmpc_debug_use_fused(mpcx_lmpc_t h, int mode);
/* 1 = always the generic (roll-out) assemble kernel, whatever the reference layout */
int mpcx_lmpc_debug_force_generic(mpcx_lmpc_t h, int on);
/* rounds the polish-only kernel may spend before an instance goes to the ADMM kernel (default 30), and the ADMM iterations
 * between two polish attempts there (default 10); rounds0 = 1 sends nearly every instance through the ADMM path            */
int mpcx_lmpc_debug_set_rounds(mpcx_lmpc_t h, int rounds0, int check_every);
/* device buffer [B x 8] of int64 receiving per-instance cycle stamps of the solve kernel (NULL: off) */
int mpcx_lmpc_debug_set_cycle_buffer(mpcx_lmpc_t h, void *dev_ptr);
/* the wave-wide sums of the lean LMPC kernels side by side, one wavefront per vector: in [nvec][64] doubles -> out [nvec][4][64] = every lane of
 * (0) the six-level butterfly sum, (1) its lane-swap / DPP form, (2) the two-level sum over lanes l, l ^ 16, l ^ 32, l ^ 48 by shuffles, (3) the same
 * by lane swaps.  Device pointers; asynchronous on `stream` */
int mpcx_lmpc_debug_wave_reduce(const double *in, double *out, int nvec, void *stream);
/* one working-set solve of the lean LMPC kernels (the Gauss-Jordan elimination on Y[A, A] and the update w = t0 - Y[:, A] lambda, one-chunk shape) per
 * wavefront, with the elimination's pivot row by scalar lane reads (form 0) and by DPP row broadcast inside the FMA (form 1).  `count` problems: Y
 * [count][n][ldy] dense symmetric (indices 0 .. nz - 1 the decision variables, nz .. n - 1 the general rows; nz and n - nz even, 2 .. 128; ldy >= n, even),
 * wsidx / wsb [count][16] the working set's indices (clamped to 0 .. n - 1) and bound values, na [count] its size (1 .. 16: it selects the size class; a
 * problem with another na is skipped), t0 [count][n] = [t0 | G t0].  out [count][2][274] per form: dep_at (position of a dependent row, or -1), lmax,
 * lam [16], w of the 64 lanes [128], G w of the 64 lanes [128]; a solve that ends at a dependent row writes only dep_at and zeros.  Device pointers;
 * asynchronous on `stream` */
int mpcx_lmpc_debug_ws_solve(const double *Y, int n, int ldy, int nz, const int *wsidx, const double *wsb, const int *na, const double *t0, double *out,
                             int count, void *stream);
/* one more replay of a loop's tick graph behind a finished run, without the reset: the tick counter stands at `ticks`, so the replay writes no
 * trajectory, state or counter / the tick counter as it stands on the device, after synchronising the device */
int mpcx_lmpc_loop_debug_replay(mpcx_lmpc_loop_t l, void *stream);
int mpcx_lmpc_loop_debug_tick(mpcx_lmpc_loop_t l, int *tick);
/* the same two for an NLMPC loop (the caller's loop of examples/vanderpol_ex.cpp:76-85 / ugv_ex.cpp on the device): one more replay of the
 * later ticks' graph behind a finished run -- the counter stands at `ticks`, the advance kernel returns before its first store -- and the
 * tick counter as it stands on the device, after synchronising the device */
int mpcx_nlmpc_loop_debug_replay(mpcx_nlmpc_loop_t l, void *stream);
int mpcx_nlmpc_loop_debug_tick(mpcx_nlmpc_loop_t l, int *tick);
/* the SQP kernel's own convergence test: step length relative to max(1, |z|) and largest constraint defect */
int mpcx_nlmpc_debug_set_tolerances(mpcx_nlmpc_t h, double tol_step, double tol_con);
/* which kernel the last solve of a built-in system went through: 0 = nlmpc_sqp (one wavefront per instance, the reduced problem in a
 * per-instance HBM workspace), 1 | 2 | 4 = nlmpc_sqp_wg (one workgroup of that many wavefronts per instance, the reduced problem in LDS);
 * -1 = none yet.  This one: the last launch of the process.  MPCX_NLMPC_FORM=wg|wave, MPCX_NLMPC_WAVES=1|2|4|8 and MPCX_NLMPC_BLOCKS=1|0 in
 * the environment force a form for the handles created afterwards (measurements, tests/test_nlmpc_forms.py). */
int mpcx_nlmpc_debug_last_form(void);
/* which form of the n x n products the following mpcx_dare_batch calls of the process take: 0 the one of the size class (the default),
 * 1 lanes over the entries, 2 the f64 matrix pipe (tools/dare_bench.py measures one against the other); returns the previous value */
int mpcx_dare_debug_product(int product);
/* the same for the last solve of this handle (the form is a property of the controller: chosen when its bounds are set, from the plan of the
 * workgroup form, the same for every batch size -- a shard of a batch takes the kernel the whole batch would; the overrides are read when
 * the handle is created) */
int mpcx_nlmpc_last_form(mpcx_nlmpc_t h);
/* one instance's slice of the SQP workspace copied to the host, with the offsets of its arrays (NlmpcWsLayout) */
int mpcx_nlmpc_debug_get_ws(mpcx_nlmpc_t h, int instance, double *out, int cap, int *layout, int nlayout);
/* user hooks given as source: the translation unit the run-time compiler is fed / a compile-only check (> 0: it builds, the size of the
 * code object; a negative MPCX_E_* code otherwise, the compiler's log through mpcx_last_error()) */
int mpcx_nlmpc_debug_generated_source(const mpcx_nlmpc_source *src, char *out, int cap);
int mpcx_nlmpc_debug_compile_source(const mpcx_nlmpc_source *src);
/* one O(n^3) array ("H", "Kinv", "Gr", "Gc", "Y", "rho_b", "rho_g"; "flags" = [cost_direct, condensed on the device]) of controller k
 * of a bank, copied to the host; out = NULL returns the length.  "fallback": the bank's failure queue, as mpcx_lmpc_debug_get's */
int mpcx_lmpc_hetero_debug_get(mpcx_lmpc_hetero_t f, int k, const char *name, double *out, int cap);

const char *mpcx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MPCX_H */
