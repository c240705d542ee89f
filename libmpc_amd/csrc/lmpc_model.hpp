// Host-side controller state and condensing for the batched LMPC path.
//
// LmpcController keeps exactly the state libmpc++'s linear front-end keeps in its
// ProblemBuilder (reference include/mpc/LMPC/ProblemBuilder.hpp:829-853) and
// LOptimizer (include/mpc/LMPC/LOptimizer.hpp:523-525): augmented model, per-step
// weights and bounds with the reference's "+1 column shift", scalar constraint,
// references, exogenous inputs, LParameters.  condense() turns it into the dense
// condensed QP in absolute inputs that the HIP kernel iterates on (SURVEY.md
// Appendix A "condensed equivalent").
#pragma once

#include <cmath>
#include <cstddef>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mpcx.h"
#include "lmpc_device.hpp"

namespace mpcx {

constexpr double kInf = std::numeric_limits<double>::infinity();

// column-major dense matrix, just enough for set-up
struct Mat {
    int r = 0, c = 0;
    std::vector<double> a;
    Mat() = default;
    Mat(int r_, int c_, double v = 0.0) : r(r_), c(c_), a((size_t)r_ * c_, v) {}
    double &operator()(int i, int j) { return a[(size_t)i + (size_t)j * r]; }
    double operator()(int i, int j) const { return a[(size_t)i + (size_t)j * r]; }
    double *col(int j) { return a.data() + (size_t)j * r; }
    const double *col(int j) const { return a.data() + (size_t)j * r; }
};

Mat matmul(const Mat &A, const Mat &B);
Mat transpose(const Mat &A);
// in-place lower Cholesky of SPD A; returns smallest pivot (<=0 on failure)
double cholesky_lower(Mat &A);
// inverse of SPD matrix from its Cholesky factor
Mat spd_inverse_from_chol(const Mat &L);

struct GeneralRow {
    int kind, step, comp;   // which functional of the predicted trajectory (GKind, lmpc_device.hpp)
    int refrow;             // row in the reference QP's inequality block numbering + neq offset applied later
    double lo, hi;          // bounds before the per-instance free-response offset
    double soft = 0.0;      // 1 / weight of a soft row, 0: hard
};

struct BoxRef {            // a reference row that bounds condensed variable `var`
    int var, refrow;
    double lo, hi;
};

struct Condensed {
    int nf = 0, nz = 0, mg = 0, ldz = 0, ldg = 0, ldy = 0;
    int n_ref = 0, m_ref = 0, neq_ref = 0, active_words = 0;
    bool has_dist = false, h_regularised = false;
    double inverse_residual = 0;                 // || H Hinv - I ||_max of the computed inverse
    std::vector<double> H, Kinv, Gr, Gc, Y;      // padded, see lmpc_device.hpp
    size_t big_n[5] = {0, 0, 0, 0, 0};           // structure-only condensing: the lengths H, Kinv, Gr, Gc, Y would have (they stay empty)
    std::vector<double> lw, uw, rho_b;           // [ldz]
    std::vector<double> lg0, ug0, rho_g;         // [ldg]
    std::vector<double> g_soft;                  // [ldg] 1 / weight of a soft general row, 0 for a hard one and for the padding
    int n_soft = 0;                              // soft general rows: by how many a working set may exceed nz
    // what LmpcDev::rho_g points to, [2 ldg]: the step sizes, then g_soft (MPCX_G_SOFT in lmpc_device.hpp reads the second half).  The one place
    // that builds the combined array: every upload of rho_g goes through it; the device condensing rewrites the first half only
    std::vector<double> rho_g_device() const
    {
        std::vector<double> v(rho_g);
        v.insert(v.end(), g_soft.begin(), g_soft.end());
        return v;
    }
    std::vector<int> g_kind, g_step, g_comp, g_refrow;      // [ldg]
    std::vector<GeneralRow> fixed_rows;          // rows that do not depend on the decision variables
    std::vector<int> boxrow_ptr, boxrow_ref;     // CSR var -> reference rows
    std::vector<double> boxrow_lo, boxrow_hi;
    std::vector<int> blk;                        // [ph+1] condensed block of v_i (blk[0] unused)
    double flops_setup = 0;

    // ---- stacked affine maps for the MFMA assemble kernel (lmpc_kernels.hip) -------------
    // input vector vin = [x0 (nxp) | u0 (nup) | yref (nyp) | 1,0,0,0], every block padded to a
    // multiple of 4 (one f64 MFMA k-step); MA rows = [f (nz16) | goff (mg16) | feasibility rows
    // (ns16) | Qc vin (kq16)], every block padded to a multiple of 16 (one MFMA row tile).
    int kin = 0, nxp = 0, nup = 0, nyp = 0, ione = 0;
    int nz16 = 0, mg16 = 0, ns = 0, ns16 = 0, kq16 = 0, rowsA = 0, ldy16 = 0;
    std::vector<double> MA[2];                   // [0]: shared yref, [1]: per-instance constant yref; rowsA x kin, column-major
    std::vector<double> slo, shi;                // [ns16] bounds of the feasibility rows
    std::vector<double> Ym;                      // -Y[:, 0:nz], ldy16 x nz16 column-major (tile padded)
    // ---- the same maps composed for the fused solve kernel: everything lmpc_solve needs of an instance is MF * vin, rows
    // [t0 ; gt0 (ldy) | goff (ldg) | f (ldz) | feasibility rows (nsp) | Qc vin (kin)], rowsF x kin column-major
    int rowsF = 0, nsp = 0;
    std::vector<double> MF[2];
};

struct AsmOut {
    std::vector<double> f, goff, sval;
    double c0 = 0;
};

struct LmpcController {
    mpcx_dims d{};
    int na = 0;
    // model
    Mat A, B, C, Bd, Dd;
    bool have_model = false;
    // ProblemBuilder state (internal columns 0..ph, see ProblemBuilder.hpp:254-260)
    Mat wOutput, wU, wDeltaU;
    Mat minX, maxX, minY, maxY, minU, maxU;
    Mat minDU, maxDU;       // [nu x ph], column i bounds delta_i (no column shift, as wDeltaU); columns past ch are kept and not read
    // soft-constraint weights of the state / output / scalar rows, internal columns as the bounds they go with; +inf: the row is hard
    Mat softX, softY;
    std::vector<double> softS;
    std::vector<double> sMin, sMax, sX, sU;
    // terminal cost 0.5 (x_ph - x_T)' P (x_ph - x_T), x_T = xT + Tx [yref(., ph - 1); dmeas(., ph - 1)] (no counterpart in the
    // reference's LMPC).  termP [nx x nx] symmetric positive semidefinite, termXT [nx], termTx [nx x (ny + ndu)]; empty without the term
    bool have_terminal = false;
    Mat termP, termTx;
    std::vector<double> termXT;
    // linear rows linLo(c, i) <= linFx(c, :) x_i + linFu(c, :) v_i <= linHi(c, i), i = 0 .. ph internal columns as sMin / sMax (no
    // counterpart in the reference's LMPC).  linFx [nlin x nx], linFu [nlin x nu] shared by all steps; linSoft [nlin x (ph + 1)]: +inf, the row is hard
    int nlin = 0;
    Mat linFx, linFu, linLo, linHi, linSoft;
    // LOptimizer state
    Mat yRef, uRef, duRef, dMeas;
    mpcx_lparams prm{};

    explicit LmpcController(const mpcx_dims &dims);

    bool pred_slice_valid(int start, int end) const;   // IMPC.hpp:251-260
    bool ctrl_slice_valid(int start, int end) const;   // IMPC.hpp:269-278

    // matrix-form setters (ProblemBuilder.hpp:247-263, 378-432)
    void set_objective(const double *OW, const double *UW, const double *DUW);
    void set_objective_idx(int idx, const double *ow, const double *uw, const double *duw);
    void set_state_bounds(const double *lo, const double *hi);
    void set_state_bounds_idx(int idx, const double *lo, const double *hi);
    void set_input_bounds(const double *lo, const double *hi);
    void set_input_bounds_idx(int idx, const double *lo, const double *hi);
    void set_output_bounds(const double *lo, const double *hi);
    void set_output_bounds_idx(int idx, const double *lo, const double *hi);
    // bounds on the input increments: the reference builds these rows and offers no setter for them (ProblemBuilder.hpp:768-793)
    void set_rate_bounds(const double *lo, const double *hi);
    void set_rate_bounds_idx(int idx, const double *lo, const double *hi);
    // weights of the penalty 0.5 rho dist^2(row value, [lo, hi]) that replaces a state / output / scalar row (no counterpart in the reference's
    // LMPC); a null pointer leaves that kind as it is.  idx form: the column shift of set_state_bounds_idx
    void set_soft_weights(const double *xw, const double *yw, const double *sw);
    void set_soft_weights_idx(int idx, const double *xw, const double *yw, const double *sw);
    // empty string, or why the term is refused (nothing is stored then).  P null: the term is removed; xT / Tx null: zeros
    std::string set_terminal_cost(const double *P, const double *xT, const double *Tx);
    // what the device reads behind the output weights (MPCX_TERMINAL in lmpc_device.hpp): [P | xT | Tx], empty without the term
    std::vector<double> terminal_block() const;
    void set_scalar_vec(const double *smin, const double *smax, const double *X, const double *U);
    void set_scalar_idx(int idx, double smin, double smax, const double *X, const double *U);

    // linear rows: empty string, or why the call is refused (nothing is stored then).  Whole horizon: lo, hi [nc x (ph + 1)] column-major, column =
    // step; nc = 0 removes the rows.  Slice [s, e) of the prediction horizon (resolved and checked by the caller): lo, hi [nc], column shift of
    // set_scalar_idx; an nc other than the stored one only while no step outside the slice holds a finite bound
    std::string set_linear(int nc, const double *Fx, const double *Fu, const double *lo, const double *hi);
    std::string set_linear_slice(int nc, const double *Fx, const double *Fu, const double *lo, const double *hi, int s, int e);
    std::string set_linear_weights(const double *w, int s, int e);       // w [nlin]; s = e = -1: steps 0 .. ph
    // what the device reads behind sX (MPCX_LINEAR_F in lmpc_device.hpp): [sX | row c: Fx(c, :) Fu(c, :)]
    std::vector<double> scalar_linear_block() const;
    // linear rows with a finite bound somewhere: zero means the controller condenses as one that never had any
    int linear_rows_live() const;

    // returns empty string on success, message otherwise
    // like != nullptr: the structure and the O(n) arrays only, rows classified as in `like` (see lmpc_model.cpp)
    std::string condense(Condensed &out, const Condensed *like = nullptr) const;
    // host evaluation of what the generic assemble kernel computes for one instance
    void assemble_host(const Condensed &o, const double *x0, const double *u0, const Mat &yR, const Mat &uR,
                       const Mat &dR, const Mat &dM, AsmOut &out) const;
    void build_fast_maps(Condensed &o) const;
    // the same after a change of references / exogenous inputs only: the constant column (and the linear part of the cost
    // form) of both maps; the quadratic part does not depend on them
    void refresh_fast_maps(Condensed &o) const;
    void compose_fused_maps(Condensed &o) const;
};

}  // namespace mpcx
